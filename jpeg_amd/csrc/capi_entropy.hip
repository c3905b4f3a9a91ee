// capi_entropy.hip -- the C ABI, device entropy unit: files whose restart intervals are Huffman-decoded by k_huffman_intervals
// (kernels_entropy.hip) into planes in device memory.  The planner and the host form of the decoder are in entropy.cpp.
#include "capi_internal.hpp"
#include "interval_plan.hpp"

using namespace jpeg_amd;
using namespace jpeg_amd::capi;

namespace {

// k_huffman_intervals between two events of the context; after the caller's wait for the stream, kernel_done adds the time.
int timed_launch(jpeg_amd_ctx *ctx, const IntervalLaunch &g)
{
    for (hipEvent_t &ev : ctx->entropy_ev)
        if (!ev) JA_HIP(ctx, hipEventCreate(&ev));
    JA_HIP(ctx, hipEventRecord(ctx->entropy_ev[0], ctx->stream));
    JA_HIP(ctx, launch_huffman_intervals(ctx->stream, g));
    JA_HIP(ctx, hipEventRecord(ctx->entropy_ev[1], ctx->stream));
    return JPEG_AMD_OK;
}
void kernel_done(jpeg_amd_ctx *ctx)
{
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->entropy_ev[0], ctx->entropy_ev[1]) == hipSuccess) ctx->device_entropy_kernel_ms += ms;
}

}  // namespace

int jpeg_amd_jpeg_decode_spectral_device(jpeg_amd_ctx *ctx, int n_images, const uint8_t *const h_jpeg[], const size_t nbytes[],
                                         int16_t *const d_coef[][JPEG_AMD_MAX_PLANES],
                                         uint16_t h_quanta[][JPEG_AMD_MAX_PLANES][64], jpeg_amd_frame_info *h_info,
                                         int32_t *h_status)
try {
    namespace iv = jpeg_amd::interval;
    if (n_images < 0) return JPEG_AMD_EINVAL;
    if (n_images > 0 && (!h_jpeg || !nbytes || !d_coef || !h_quanta || !h_info || !h_status)) return JPEG_AMD_EINVAL;
    for (int i = 0; i < n_images; ++i)
        if (!h_jpeg[i]) return JPEG_AMD_EINVAL;
    // everything that headers and marker positions decide, for every file, before anything is enqueued
    std::vector<iv::FilePlan> plans((size_t)n_images);
    std::vector<iv::FileBlock> blocks((size_t)n_images);
    std::vector<uint32_t> first((size_t)n_images + 1, 0);
    size_t blocks_bytes = 0;
    for (int i = 0; i < n_images; ++i) {
        JA_TRY(iv::plan_file(h_jpeg[i], nbytes[i], &plans[i]));
        for (int c = 0; c < plans[i].info.ncomponents; ++c)
            if (!d_coef[i][c] || reinterpret_cast<uintptr_t>(d_coef[i][c]) % 16) return JPEG_AMD_EINVAL;
        for (const iv::IntervalWork &w : plans[i].work)
            if (!iv::work_fits(w, plans[i].scans[w.scan], nbytes[i])) return JPEG_AMD_EINVAL;
        blocks[i] = iv::file_block(plans[i]);
        blocks_bytes += blocks[i].size;
        if (plans[i].work.size() > 0xffffffffu - first[i]) return JPEG_AMD_ENOSUP;     // (a launch counts its work-items in 32 bits)
        first[i + 1] = first[i] + (uint32_t)plans[i].work.size();
    }
    JA_TRY(bind(ctx));
    if (n_images == 0) return JPEG_AMD_OK;

    // one buffer: [the files' records][the prefix of their intervals][their blocks] and, behind what is uploaded, the statuses
    const size_t files_at = 0, first_at = align256(sizeof(iv::IntervalFile) * n_images);
    const size_t blocks_at = first_at + align256(sizeof(uint32_t) * (n_images + 1));
    const size_t status_at = align256(blocks_at + blocks_bytes), nwork = first[n_images];
    std::vector<char> host(status_at);
    size_t at = blocks_at;
    for (int i = 0; i < n_images; ++i) {
        const iv::IntervalFile f = iv::file_record(plans[i], blocks[i], at, d_coef[i]);
        std::memcpy(host.data() + files_at + sizeof f * i, &f, sizeof f);
        iv::write_file_block(plans[i], blocks[i], h_jpeg[i], host.data() + at);
        at += blocks[i].size;
    }
    std::memcpy(host.data() + first_at, first.data(), sizeof(uint32_t) * first.size());
    JA_TRY(ensure_buffer(ctx, ctx->entropy, status_at + sizeof(int32_t) * nwork));
    char *dev = static_cast<char *>(ctx->entropy.ptr);
    JA_HIP(ctx, hipMemcpyAsync(dev, host.data(), status_at, hipMemcpyHostToDevice, ctx->stream));
    IntervalLaunch g{};
    g.base = reinterpret_cast<const uint8_t *>(dev);
    g.files = reinterpret_cast<const iv::IntervalFile *>(dev + files_at);
    g.first = reinterpret_cast<const uint32_t *>(dev + first_at);
    g.status = reinterpret_cast<int32_t *>(dev + status_at);
    g.base_bytes = status_at;
    g.nfiles = (uint32_t)n_images;
    g.nwork = (uint32_t)nwork;
    JA_TRY(timed_launch(ctx, g));
    std::vector<int32_t> status(nwork);
    JA_HIP(ctx, hipMemcpyAsync(status.data(), g.status, sizeof(int32_t) * nwork, hipMemcpyDeviceToHost, ctx->stream));
    JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    kernel_done(ctx);
    ctx->device_entropy_files += n_images;

    int result = JPEG_AMD_OK;
    for (int i = 0; i < n_images; ++i) {
        h_status[i] = JPEG_AMD_OK;
        for (uint32_t k = first[i]; k < first[i + 1] && h_status[i] == JPEG_AMD_OK; ++k) h_status[i] = status[k];
        if (result == JPEG_AMD_OK) result = h_status[i];
        std::memcpy(h_quanta[i], plans[i].quanta, sizeof plans[i].quanta);
        h_info[i] = plans[i].info;
    }
    return result;
}
JA_NOTHROW_TAIL

int jpeg_amd::capi::decode_blocks_on_device(jpeg_amd_ctx *ctx, const DeviceEntropyJob *jobs, int n)
{
    namespace iv = jpeg_amd::interval;
    if (n <= 0) return JPEG_AMD_OK;
    // [the files' records][the prefix of their intervals][their blocks] and, behind them, the statuses
    const size_t first_at = align256(sizeof(iv::IntervalFile) * n), blocks_at = first_at + align256(sizeof(uint32_t) * (n + 1));
    std::vector<char> head(blocks_at);
    std::vector<size_t> block_at((size_t)n);
    std::vector<uint32_t> first((size_t)n + 1, 0);
    size_t at = blocks_at;
    for (int i = 0; i < n; ++i) {
        iv::IntervalFile f = jobs[i].file->record;
        block_at[i] = at;
        f.scans_at += at; f.tables_at += at; f.work_at += at; f.bytes_at += at;
        for (int c = 0; c < JPEG_AMD_MAX_PLANES; ++c) f.plane[c] = jobs[i].d_planes[c];
        std::memcpy(head.data() + sizeof f * i, &f, sizeof f);
        if (f.nwork > 0xffffffffu - first[i]) return JPEG_AMD_ENOSUP;
        first[i + 1] = first[i] + f.nwork;
        at += align256(jobs[i].file->bytes);
    }
    std::memcpy(head.data() + first_at, first.data(), sizeof(uint32_t) * first.size());
    const size_t status_at = at, nwork = first[n];
    JA_TRY(ensure_buffer(ctx, ctx->entropy, status_at + sizeof(int32_t) * nwork));
    char *dev = static_cast<char *>(ctx->entropy.ptr);
    JA_HIP(ctx, hipMemcpyAsync(dev, head.data(), blocks_at, hipMemcpyHostToDevice, ctx->stream));
    for (int i = 0; i < n; ++i)
        JA_HIP(ctx, hipMemcpyAsync(dev + block_at[i], jobs[i].h_block, jobs[i].file->bytes, hipMemcpyHostToDevice, ctx->stream));
    IntervalLaunch g{};
    g.base = reinterpret_cast<const uint8_t *>(dev);
    g.files = reinterpret_cast<const iv::IntervalFile *>(dev);
    g.first = reinterpret_cast<const uint32_t *>(dev + first_at);
    g.status = reinterpret_cast<int32_t *>(dev + status_at);
    g.base_bytes = status_at;
    g.nfiles = (uint32_t)n;
    g.nwork = (uint32_t)nwork;
    JA_TRY(timed_launch(ctx, g));
    std::vector<int32_t> status(nwork);
    JA_HIP(ctx, hipMemcpyAsync(status.data(), g.status, sizeof(int32_t) * nwork, hipMemcpyDeviceToHost, ctx->stream));
    JA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    kernel_done(ctx);
    ctx->device_entropy_files += n;
    for (int32_t st : status)
        if (st != JPEG_AMD_OK) return st;
    return JPEG_AMD_OK;
}

int jpeg_amd_ctx_device_entropy_files(const jpeg_amd_ctx *ctx, int64_t *count)
{
    if (!ctx || !count) return JPEG_AMD_EINVAL;
    *count = ctx->device_entropy_files;
    return JPEG_AMD_OK;
}

int jpeg_amd_ctx_device_entropy_kernel_ms(const jpeg_amd_ctx *ctx, double *ms)
{
    if (!ctx || !ms) return JPEG_AMD_EINVAL;
    *ms = ctx->device_entropy_kernel_ms;
    return JPEG_AMD_OK;
}
