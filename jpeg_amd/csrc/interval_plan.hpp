// interval_plan.hpp -- the work list of the device entropy decoder for one file, as the planner (entropy.cpp) builds it on the
// host, and the file's block of a launch's buffer: the scans, tables and intervals of huffman_interval.hpp and the file's
// entropy-coded bytes, one behind the other, with every offset counted from the block's own parts -- so a block can be written
// anywhere (by any thread) and found through the file's IntervalFile record alone.  Host only.
#pragma once

#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/jpeg_amd.h"
#include "huffman_interval.hpp"

namespace jpeg_amd {
namespace interval {

struct ScanBytes {
    size_t begin, end;                      // the scan's entropy-coded segment, offsets in the file
};
struct FilePlan {
    jpeg_amd_frame_info info{};
    uint16_t quanta[JPEG_AMD_MAX_PLANES][64] = {};
    std::vector<IntervalTable> tables;      // every distinct table a scan of the file uses
    std::vector<IntervalScan> scans;        // td and ta index `tables`
    std::vector<ScanBytes> bytes;           // per scan
    std::vector<IntervalWork> work;         // scan indexes `scans`; begin and end are offsets in the FILE, inside bytes[scan]
};

// The planner's verdict on a file (include/jpeg_amd.h, jpeg_amd_jpeg_plan_intervals) and, with JPEG_AMD_OK, its work list.
// Throws what its vectors throw.
int plan_file(const uint8_t *data, size_t nbytes, FilePlan *plan);

// What is checked of every interval before a byte of it is read: MCUs inside the scan, bytes inside the buffer.
inline bool work_fits(const IntervalWork &w, const IntervalScan &s, size_t nbytes)
{
    return w.mcu0 <= w.mcu1 && w.mcu1 <= (uint32_t)s.mcus && w.begin <= w.end && w.end <= nbytes;
}

// Where the parts of a file's block begin, from the block's first byte, and its size (a multiple of 16).
struct FileBlock {
    size_t scans_at, tables_at, work_at, bytes_at, nbytes, size;
};
inline FileBlock file_block(const FilePlan &p)
{
    FileBlock b{};
    b.scans_at = 0;
    b.tables_at = b.scans_at + p.scans.size() * sizeof(IntervalScan);
    b.work_at = b.tables_at + p.tables.size() * sizeof(IntervalTable);
    b.bytes_at = b.work_at + p.work.size() * sizeof(IntervalWork);
    for (const ScanBytes &s : p.bytes) b.nbytes += s.end - s.begin;
    b.size = (b.bytes_at + b.nbytes + 15) & ~(size_t)15;
    return b;
}
// The block of the file `data` at dst (b.size bytes): the scans' segments one behind the other, the intervals' byte ranges
// counted from the first of them.
inline void write_file_block(const FilePlan &p, const FileBlock &b, const uint8_t *data, char *dst)
{
    if (!p.scans.empty()) std::memcpy(dst + b.scans_at, p.scans.data(), p.scans.size() * sizeof(IntervalScan));
    if (!p.tables.empty()) std::memcpy(dst + b.tables_at, p.tables.data(), p.tables.size() * sizeof(IntervalTable));
    std::vector<size_t> segment_at(p.bytes.size());
    size_t at = 0;
    for (size_t k = 0; k < p.bytes.size(); ++k) {
        segment_at[k] = at;
        std::memcpy(dst + b.bytes_at + at, data + p.bytes[k].begin, p.bytes[k].end - p.bytes[k].begin);
        at += p.bytes[k].end - p.bytes[k].begin;
    }
    std::memset(dst + b.bytes_at + at, 0, b.size - b.bytes_at - at);
    for (size_t k = 0; k < p.work.size(); ++k) {
        IntervalWork w = p.work[k];
        const size_t shift = p.bytes[w.scan].begin - segment_at[w.scan];
        w.begin -= shift;
        w.end -= shift;
        std::memcpy(dst + b.work_at + k * sizeof w, &w, sizeof w);
    }
}
// The file's record for a block that lies `block_at` bytes behind the launch's base.
inline IntervalFile file_record(const FilePlan &p, const FileBlock &b, size_t block_at, int16_t *const planes[])
{
    IntervalFile f{};
    for (int c = 0; c < p.info.ncomponents; ++c) f.plane[c] = planes[c];
    f.scans_at = block_at + b.scans_at;
    f.tables_at = block_at + b.tables_at;
    f.work_at = block_at + b.work_at;
    f.bytes_at = block_at + b.bytes_at;
    f.nbytes = b.nbytes;
    f.nscans = (uint32_t)p.scans.size();
    f.ntables = (uint32_t)p.tables.size();
    f.nwork = (uint32_t)p.work.size();
    return f;
}

}  // namespace interval
}  // namespace jpeg_amd
