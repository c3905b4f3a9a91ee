// kernels_entropy.hip -- Huffman entropy decoding on the device: k_huffman_intervals, one restart interval per work-item.
//
// The restart intervals of a sequential scan are independent bit streams (T.81 E.2.4): each starts on a byte boundary with its
// predictors at zero and writes blocks no other interval writes.  The host plans the work (entropy.cpp, plan_file: one
// IntervalWork per interval of every scan of every file of the launch) and uploads the entropy-coded bytes, the Huffman tables
// and the scan records; a work-item runs huffman_interval.hpp's decode_interval, the very text the host instantiates in
// jpeg_amd_jpeg_decode_intervals_host, and writes its interval's status with an ordinary store.
//
// A lane walks a serial chain of table lookups, and the lanes of a wave walk different streams: every load is divergent.  The
// tables (1488 bytes each, a handful per file) stay in global memory, where the first level of the files in flight lives in the
// vector L1 and L2; LDS copies would have to be per file, and a workgroup's intervals may belong to several files.  A block's
// 64 coefficients are indexed by the stream, so they are not kept in registers (that would be scratch): the lane zeroes the
// block in its plane with eight 16-byte stores and scatters the few coefficients behind them -- same lane, same addresses, program
// order.  Workgroups of one wave: nothing is shared between lanes, and small groups spread a launch of a few thousand
// intervals over more compute units.
//
// Every index the kernel takes from device memory is clamped or checked against the launch's own counts before it is used
// (the host has checked the same before the upload: interval_plan.hpp, work_fits), and huffman_interval.hpp bounds what the
// stream's contents can do.
#include "kernels.hpp"
#include "huffman_interval.hpp"

namespace jpeg_amd {

namespace {

constexpr int kThreads = 64;

__global__ __launch_bounds__(kThreads) void k_huffman_intervals(IntervalLaunch g)
{
    using namespace interval;
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= g.nwork) return;
    // the interval's file: the last f with first[f] <= i (a file without intervals is never found)
    uint32_t lo = 0, hi = g.nfiles;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (g.first[mid] <= i) lo = mid; else hi = mid;
    }
    const IntervalFile &f = g.files[lo];
    const uint32_t k = i - g.first[lo];
    int st = kInvalid;
    // the file's block lies inside the buffer, part by part (every size is 32 bits times a small constant: no overflow)
    const bool block_fits = f.scans_at <= g.base_bytes && (uint64_t)f.nscans * sizeof(IntervalScan) <= g.base_bytes - f.scans_at &&
                            f.tables_at <= g.base_bytes && (uint64_t)f.ntables * sizeof(IntervalTable) <= g.base_bytes - f.tables_at &&
                            f.work_at <= g.base_bytes && (uint64_t)f.nwork * sizeof(IntervalWork) <= g.base_bytes - f.work_at &&
                            f.bytes_at <= g.base_bytes && f.nbytes <= g.base_bytes - f.bytes_at &&
                            ((f.scans_at | f.tables_at | f.work_at) & 15) == 0;
    if (block_fits && k < f.nwork) {
        const IntervalWork w = reinterpret_cast<const IntervalWork *>(g.base + f.work_at)[k];
        if (w.scan < f.nscans) {
            const IntervalScan &s = reinterpret_cast<const IntervalScan *>(g.base + f.scans_at)[w.scan];
            bool fits = s.ns >= 1 && s.ns <= 4 && s.mcux >= 1 && s.mcus >= 1;
            for (int j = 0; j < 4; ++j)
                if (j < s.ns) fits = fits && (uint32_t)s.c[j].td < f.ntables && (uint32_t)s.c[j].ta < f.ntables && s.c[j].ux >= 0 && s.c[j].uy >= 0;
            if (fits) {
                const uint8_t *bytes = g.base + f.bytes_at;
                const uint64_t end = w.end < f.nbytes ? w.end : f.nbytes, begin = w.begin < end ? w.begin : end;
                const uint32_t mcu1 = w.mcu1 < (uint32_t)s.mcus ? w.mcu1 : (uint32_t)s.mcus;
                st = decode_interval(s, reinterpret_cast<const IntervalTable *>(g.base + f.tables_at), f.plane, bytes + begin,
                                     bytes + end, w.mcu0, mcu1);
            }
        }
    }
    g.status[i] = st;
}

}  // namespace

hipError_t launch_huffman_intervals(hipStream_t stream, const IntervalLaunch &g)
{
    if (g.nwork == 0) return hipSuccess;
    hipLaunchKernelGGL(k_huffman_intervals, dim3((g.nwork + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, g);
    return hipGetLastError();
}

}  // namespace jpeg_amd
