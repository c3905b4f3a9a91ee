// kernels_expand.hip -- sparse coefficients -> the parts of the planes that a view reads (jpeg_amd_spectral_expand_mixed and
// the file calls of capi_files.hip): k_expand_sparse (kernels_stage.hip) for images of DIFFERENT geometries in one launch,
// restricted per plane to a window of blocks and per block to its leading octets.
//
// k_expand_mixed: the work-items of all images laid end to end, a prefix table mapping a workgroup to its image as in the
// mixed tile kernel (tile_decode.hpp, rect_image), the image's geometry in a record in device memory.  A work-item rebuilds
// ONE 16-byte octet (eight coefficients in zigzag order) of one block of a window and stores it with one 16-byte store, as
// k_expand_sparse does.  With a head of h octets a block takes h consecutive work-items, so a workgroup holds 256 / h blocks
// and no lane idles behind a short head: 256 blocks at h = 1, 64 at h = 4, 32 at h = 8.  The blocks of a window are numbered
// row by row, so the work-items of a wave write neighbouring blocks of one block row: at h = 8 a wave writes 1 KiB in a row, at
// h = 4 the first half and at h = 1 the first eighth of each 128-byte block -- the planes keep their pitch, so a short head
// can fill no more of a line than that; what it saves is the other bytes of the line and the entries behind the head.
// The walk relies on the order of a block's entries (sparse_format.hpp): it stops at the first entry at or behind 8 * head, or
// at the last-entry flag, whichever comes first.  Entries behind the head are not read beyond that one.
#include "kernels.hpp"
#include "sparse_format.hpp"

#include <cstring>

namespace jpeg_amd {

namespace {

constexpr int kThreads = 256;

// One image of a launch, written by expand_mixed_record on the host.
struct ExpandMixedRecord {
    uint64_t desc_at, entries_at;                    // elements into the launch's packed records
    int16_t *coef[JPEG_AMD_MAX_PLANES];
    uint32_t desc_first[JPEG_AMD_MAX_PLANES];        // the plane's block (0, 0) among the image's descriptors
    uint32_t win_first[JPEG_AMD_MAX_PLANES + 1];     // the windows' blocks before plane p's; [nplanes ..]: all of them
    int32_t x[JPEG_AMD_MAX_PLANES], y[JPEG_AMD_MAX_PLANES], w[JPEG_AMD_MAX_PLANES];   // the window's origin and width, blocks
    int32_t units_x[JPEG_AMD_MAX_PLANES];            // the plane's pitch, blocks
    uint32_t shift;                                  // log2(head): 0, 2 or 3
    uint32_t reserved[2];
};
static_assert(sizeof(ExpandMixedRecord) % 16 == 0, "records lie in an array that the host stages as bytes");

struct ExpandMixedArgs {
    const ExpandMixedRecord *records;   // [n]
    const uint32_t *groups;             // [n + 1]: the prefix of the images' workgroups
    const uint32_t *packed;             // descriptors and entries of every image
    int n_images;
};

__global__ __launch_bounds__(kThreads) void k_expand_mixed(ExpandMixedArgs g)
{
    // the workgroup's image: the last i with groups[i] <= wg (an image without work has no workgroup and is never found)
    const uint32_t wg = blockIdx.x;
    int lo = 0, hi = g.n_images;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (g.groups[mid] <= wg) lo = mid; else hi = mid;
    }
    const ExpandMixedRecord &r = g.records[lo];
    const uint32_t shift = r.shift;
    const uint64_t item = (uint64_t)(wg - g.groups[lo]) * kThreads + threadIdx.x;   // (2^31 workgroups of 256: not 32 bits)
    const uint64_t jj = item >> shift;
    if (jj >= r.win_first[JPEG_AMD_MAX_PLANES]) return;
    const uint32_t j = (uint32_t)jj, octet = (uint32_t)item & ((1u << shift) - 1u);
    int p = 0;
#pragma unroll
    for (int q = 1; q < JPEG_AMD_MAX_PLANES; ++q) p += (j >= r.win_first[q]);
    // block k of plane p's window, row by row
    const uint32_t k = j - r.win_first[p], ww = (uint32_t)r.w[p];
    const uint32_t by = k / ww, bx = k - by * ww;
    const uint32_t block = ((uint32_t)r.y[p] + by) * (uint32_t)r.units_x[p] + (uint32_t)r.x[p] + bx;
    uint32_t w[4] = {0, 0, 0, 0};
    uint32_t at = g.packed[r.desc_at + r.desc_first[p] + block];
    if (at != sparse::kAbsent) {
        const uint32_t *e = g.packed + r.entries_at;
        const uint32_t end = 8u << shift;                 // the first zigzag index behind the head
        for (;; ++at) {
            const uint32_t v = e[at];
            const uint32_t pos = sparse::zigzag(v);
            if (pos >= end) break;                        // ascending: nothing of the head follows
            if ((pos >> 3) == octet) {
                const uint32_t half = (pos & 1) * 16, word = (pos >> 1) & 3;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (word == (uint32_t)i) w[i] = (w[i] & ~(sparse::kValueMask << half)) | (sparse::value(v) << half);
            }
            if (sparse::is_last(v)) break;
        }
    }
    *reinterpret_cast<uint4 *>(r.coef[p] + (size_t)block * 64 + 8 * octet) = make_uint4(w[0], w[1], w[2], w[3]);
}

uint32_t head_shift(int head) { return head == 1 ? 0u : head == 4 ? 2u : 3u; }

}  // namespace

size_t expand_mixed_record_bytes() { return sizeof(ExpandMixedRecord); }

uint64_t expand_mixed_groups(const jpeg_amd_expand_item &it)
{
    uint64_t blocks = 0;
    for (int p = 0; p < it.layout.nplanes; ++p) blocks += (uint64_t)it.window[p].width * (uint64_t)it.window[p].height;
    return ((blocks << head_shift(it.head)) + kThreads - 1) / kThreads;
}

void expand_mixed_record(void *dst, const jpeg_amd_expand_item &it)
{
    ExpandMixedRecord r{};
    r.desc_at = it.desc_at; r.entries_at = it.entries_at;
    r.shift = head_shift(it.head);
    uint32_t blocks = 0, windowed = 0;
    for (int p = 0; p < it.layout.nplanes; ++p) {
        const jpeg_amd_region &win = it.window[p];
        r.coef[p] = it.d_coef[p];
        r.desc_first[p] = blocks;
        r.win_first[p] = windowed;
        r.x[p] = win.x; r.y[p] = win.y; r.w[p] = win.width;
        r.units_x[p] = it.layout.units_x[p];
        blocks += (uint32_t)it.layout.units_x[p] * (uint32_t)it.layout.units_y[p];
        windowed += (uint32_t)win.width * (uint32_t)win.height;
    }
    for (int p = it.layout.nplanes; p <= JPEG_AMD_MAX_PLANES; ++p) r.win_first[p] = windowed;
    memcpy(dst, &r, sizeof r);
}

hipError_t launch_expand_mixed(hipStream_t stream, int n_images, const void *d_items, const uint32_t *d_groups, uint32_t nwg,
                               const uint32_t *d_records)
{
    if (n_images == 0 || nwg == 0) return hipSuccess;
    const ExpandMixedArgs g{static_cast<const ExpandMixedRecord *>(d_items), d_groups, d_records, n_images};
    hipLaunchKernelGGL(k_expand_mixed, dim3(nwg), dim3(kThreads), 0, stream, g);
    return hipGetLastError();
}

}  // namespace jpeg_amd
