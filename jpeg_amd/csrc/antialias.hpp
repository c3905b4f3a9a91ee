// antialias.hpp -- the antialiasing filter of include/jpeg_amd.h ("antialiased resample") and the walk that applies it, for
// k_tables_bytes and k_tables_tensor (kernels_resample.hip): the triangle filter widened by the scale factor, whose
// footprint per output pixel is up to 33 x 33 source pixels.  The tile, the grid and the head of the arguments are
// resample.hpp's: (tiles of 64 x 32 output pixels) x (images), no prefix and no search.
//
// The same walk applies the filter of "bicubic resample" (the same kernels): the Keys cubic widened by the scale factor, whose
// support is twice as wide, so the host's limit for it is half as large (kBicubicMaxScale) and the tables, the footprint
// and the LDS are what they are for the triangle at twice the scale factor.  The filter is a type (TriangleFilter,
// BicubicFilter): the tap loop of the contracts, antialias_taps, exists once.
//
// antialias_walk: the workgroup of a tile
//   1. TABLES.  Writes the tile's per-column and per-row (lo, count, W[count]) into LDS, one work-item per column or row: the
//      weights, their ascending sum and the one division per weight happen here and nowhere else.  The column table is written
//      for the SOURCE column of the stored pixel (xs = flip ? out_w - 1 - x : x), so a flipped image costs nothing per pixel.
//      Columns and rows of an edge tile that lie past the output get a count of 0: they read nothing and reach no sink.
//   2. SOURCE ROWS IN CHUNKS.  lo and lo + count do not decrease with the output index (every operation that makes them is
//      monotonic in binary32), so the tile's vertical footprint is [lo of its first row, lo + count of its last row).  The
//      workgroup walks those source rows in ascending order, kChunk at a time:
//        a. horizontal pass: wave v computes h(row, column, channel) of the chunk's rows v, v + 4, ... for the tile's 64
//           columns, one column per lane (byte loads; neighbouring lanes share the lines), tap by tap in ascending order, a
//           product and then a sum, and writes them to LDS [row][channel][column] (consecutive lanes, consecutive banks);
//        b. after a barrier, vertical pass: every work-item owns one column of 8 consecutive output rows (wave v: rows 8 v ...
//           8 v + 7) and adds Wy * h into 24 register accumulators, for each of its rows over that row's taps inside the
//           chunk.  Ascending source rows inside a chunk and ascending chunks are the contract's order; h is computed once per
//           source row and column, whatever the number of output rows that read it.
//      At k = 2 a tile's footprint is about 132 x 68 source pixels (3 chunks), at k = 16 1 056 x 544 (17 chunks).
//   3. STORES.  The accumulators become bytes (clamp, + 0.5, truncate), go through LDS (the chunk buffer, free by then) and
//      leave as resample_walk's runs: sink(o, y, x, npix) for 4 pixels of one row per work-item, 16 work-items across.
// Reads stay inside the image: lo >= 0 and lo + count <= n on both axes.  The count is clamped to kAntialiasMaxTaps, the
// tables' width, whatever the record says; the host refuses k > kAntialiasMaxScale (the cubic: kBicubicMaxScale), below which
// the clamp never binds.
//
// LDS: tables (64 + 32) x (33 + 2) x 4 = 13 440 bytes, chunk buffer 32 x 3 x 64 x 4 = 24 576 bytes; 38 016 in all, four
// workgroups per CU.
//
// Compile with -ffp-contract=off (see dct.hpp): every statement below is one binary32 operation.  The division is hipcc's
// default for HIP, correctly rounded (no fast-math, no -fhip-fp32-correctly-rounded-divide-sqrt=off).
#pragma once
#pragma clang fp contract(off)

#include <type_traits>

#include "fused_common.hpp"
#include "kernels.hpp"
#include "resample.hpp"

namespace jpeg_amd {

constexpr int kChunk = 32;                        // source rows per chunk
constexpr int kWaves = kThreads / kTileW;         // one column per lane in the horizontal pass
constexpr int kChunkRows = kChunk / kWaves;       // source rows per wave and chunk
constexpr int kOwnRows = kTileH / kWaves;         // output rows per work-item in the vertical pass
static_assert(kThreads == kWaves * kTileW && kChunk % kWaves == 0 && kTileH % kWaves == 0, "roles");
static_assert(kChunk * 3 * kTileW * sizeof(float) >= (size_t)3 * kTileW * kTileH, "the byte tile lies in the chunk buffer");

// The weight functions that fill the tables: the half-width of the support for s = max(k, 1), and the weight at u, the
// distance from the centre in units of s.  The walk below is written once and takes either.
struct TriangleFilter {   // "antialiased resample"
    static __device__ __forceinline__ float support(float s) { return s; }
    static __device__ __forceinline__ float weight(float u) { return fmaxf(1.0f - fabsf(u), 0.0f); }
};
struct BicubicFilter {    // "bicubic resample": the Keys cubic with a = -0.5; five operations inside 1, six inside 2
    static __device__ __forceinline__ float support(float s) { return 2.0f * s; }
    static __device__ __forceinline__ float weight(float u)
    {
        const float x = fabsf(u);
        if (x < 1.0f) return ((1.5f * x - 2.5f) * x) * x + 1.0f;
        if (x < 2.0f) return ((((x - 5.0f) * x + 8.0f) * x) - 4.0f) * -0.5f;
        return 0.0f;
    }
};

// One axis of the contract: output index j of an axis of n source samples.  W: the row of the table.
template <typename Filter>
__device__ __forceinline__ void antialias_taps(int j, float k, float s, float r, int n, int &lo, int &count, float *W)
{
    const float c = ((float)j + 0.5f) * k;
    const float p = Filter::support(s);
    lo = max((int)((c - p) + 0.5f), 0);
    const int hi = min((int)((c + p) + 0.5f), n);
    count = min(max(hi - lo, 0), kAntialiasMaxTaps);
    float total = 0.0f;
    for (int i = 0; i < count; ++i) {
        const float u = (((float)(lo + i) - c) + 0.5f) * r;
        const float w = Filter::weight(u);
        W[i] = w;
        total = i == 0 ? w : total + w;
    }
    for (int i = 0; i < count; ++i) W[i] = W[i] / total;
}

__device__ __forceinline__ uint32_t antialias_byte(float v) { return (uint32_t)(int)(fminf(fmaxf(v, 0.0f), 255.0f) + 0.5f); }

// The tile blockIdx.x of image blockIdx.y, with resample_walk's sink.  a.records is not read: the records are `records`.
// Oriented (Record = OrientedAntialiasRecord, "oriented resample"): w and h are the ORIENTED image's, offset its first byte,
// and the byte of channel c of its pixel (x', y') lies at offset + x' step_x + y' step_y + c, the steps signed: the
// horizontal pass runs along oriented x, and the vertical pass never sees the difference.
// Placed (Record = PlacedAntialiasRecord, "placed resample", oriented as well): canvas column xs = flip ? out_w - 1 - x : x takes
// the taps of xs - x0 where that lies in [0, ww) and is padded otherwise (lo = -1, count 0: it reads nothing and adds nothing);
// rows likewise.  The vertical footprint runs from the lo of the tile's first WINDOW row to lo + count of its last one -- a
// padded row has no lo -- and is empty for a tile without a window pixel, which then reads no source byte; the footprint
// follows from the record and the tile alone, so every work-item of the workgroup makes the same trips and meets the same
// barriers.  A padded pixel's bytes in the byte tile are `fill`'s (channel c in bits 8 c ...), in front of the sink.
template <typename Filter, typename Record, typename Sink>
__device__ __forceinline__ void antialias_walk(const ResampleArgs &a, const Record *records, bool flips, Sink sink, uint32_t fill = 0u)
{
    constexpr bool Placed = std::is_same<Record, PlacedAntialiasRecord>::value;
    constexpr bool Oriented = Placed || std::is_same<Record, OrientedAntialiasRecord>::value;
    using Step = typename std::conditional<Oriented, int64_t, size_t>::type;   // (the additions wrap to the same address)
    __shared__ int tlo[kTileW + kTileH], tcount[kTileW + kTileH];   // columns, then rows
    __shared__ float tw[kTileW + kTileH][kAntialiasMaxTaps];
    __shared__ float hbuf[kChunk * 3 * kTileW];

    const int t = threadIdx.x;
    uint32_t txi;
    const uint32_t tyi = a.tiles_x.div(blockIdx.x, txi);
    const int px0 = kTileW * (int)txi, py0 = kTileH * (int)tyi;
    const Record r = records[blockIdx.y];
    const bool flip = flips && r.flip;
    if (t < kTileW) {
        int lo = 0, count = 0;
        if constexpr (Placed) {
            const int xs = (flip ? a.out_w - 1 - (px0 + t) : px0 + t) - r.x0;   // (past the output: padded, and reaches no sink)
            if (xs >= 0 && xs < r.ww) antialias_taps<Filter>(xs, r.kx, r.sx, r.rx, r.w, lo, count, tw[t]);
            else lo = -1;
        } else {
            if (px0 + t < a.out_w) antialias_taps<Filter>(flip ? a.out_w - 1 - (px0 + t) : px0 + t, r.kx, r.sx, r.rx, r.w, lo, count, tw[t]);
        }
        tlo[t] = lo; tcount[t] = count;
    } else if (t < kTileW + kTileH) {
        int lo = 0, count = 0;
        if constexpr (Placed) {
            const int ys = py0 + (t - kTileW) - r.y0;
            if (ys >= 0 && ys < r.wh) antialias_taps<Filter>(ys, r.ky, r.sy, r.ry, r.h, lo, count, tw[t]);
            else lo = -1;
        } else {
            if (py0 + (t - kTileW) < a.out_h) antialias_taps<Filter>(py0 + (t - kTileW), r.ky, r.sy, r.ry, r.h, lo, count, tw[t]);
        }
        tlo[t] = lo; tcount[t] = count;
    }
    __syncthreads();

    const int col = t % kTileW, wave = t / kTileW;
    const int rows = min(kTileH, a.out_h - py0);   // of the tile, >= 1
    int first = 0, last = rows - 1;                // the tile's rows that bound the footprint
    int wrow0 = 0, wrow1 = kTileH;                 // Placed: the tile's window rows, [wrow0, wrow1)
    bool any = true;
    if constexpr (Placed) {
        wrow0 = max(py0, r.y0) - py0;
        wrow1 = min(py0 + rows, r.y0 + r.wh) - py0;
        const int c0 = flip ? a.out_w - kTileW - px0 : px0;   // the canvas columns of the tile: [c0, c0 + kTileW)
        any = wrow0 < wrow1 && max(c0, r.x0) < min(c0 + kTileW, r.x0 + r.ww);
        first = any ? wrow0 : 0;
        last = any ? wrow1 - 1 : 0;
    }
    const int ybeg = any ? tlo[kTileW + first] : 0, yend = any ? tlo[kTileW + last] + tcount[kTileW + last] : 0;
    const int xcount = tcount[col];
    const bool cpad = Placed && tlo[col] < 0;
    Step pixel_bytes = 3, row_bytes = (Step)3 * (uint32_t)r.w;
    if constexpr (Oriented) {
        pixel_bytes = r.step_x;
        row_bytes = r.step_y;
    }
    const uint8_t *src = a.src + r.offset + pixel_bytes * (uint32_t)tlo[col];
    const float *wx = tw[col];
    float acc[kOwnRows][3];
#pragma unroll
    for (int i = 0; i < kOwnRows; ++i)
        acc[i][0] = acc[i][1] = acc[i][2] = 0.0f;

    for (int y0 = ybeg; y0 < yend; y0 += kChunk) {   // the same trips for every work-item: the barriers are inside
        float h[kChunkRows][3];
#pragma unroll
        for (int i = 0; i < kChunkRows; ++i)
            h[i][0] = h[i][1] = h[i][2] = 0.0f;
        for (int k = 0; k < xcount; ++k) {
            const float w = wx[k];
#pragma unroll
            for (int i = 0; i < kChunkRows; ++i) {
                const int y = y0 + wave + kWaves * i;
                if (y < yend) {
                    const uint8_t *p = src + (Step)(uint32_t)y * row_bytes + (Oriented ? pixel_bytes * k : (Step)(3 * k));
#pragma unroll
                    for (int c = 0; c < 3; ++c) h[i][c] = h[i][c] + w * (float)p[c];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < kChunkRows; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) hbuf[((wave + kWaves * i) * 3 + c) * kTileW + col] = h[i][c];
        __syncthreads();
        const int yc = min(y0 + kChunk, yend);
#pragma unroll
        for (int i = 0; i < kOwnRows; ++i) {
            const int u = kTileW + kOwnRows * wave + i;
            const int lo = tlo[u];
            const int e = min(lo + tcount[u], yc);
            for (int y = max(lo, y0); y < e; ++y) {
                const float w = tw[u][y - lo];
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[i][c] = acc[i][c] + w * hbuf[((y - y0) * 3 + c) * kTileW + col];
            }
        }
        __syncthreads();
    }

    uint8_t *tile = reinterpret_cast<uint8_t *>(hbuf);   // [kTileH][3 kTileW]: every read of the last chunk is behind a barrier
#pragma unroll
    for (int i = 0; i < kOwnRows; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint32_t b = antialias_byte(acc[i][c]);
            if constexpr (Placed) {   // a select, not a branch: the row's verdict is the wave's, the column's the work-item's
                const bool pad = cpad || kOwnRows * wave + i < wrow0 || kOwnRows * wave + i >= wrow1;
                b = pad ? (fill >> (8 * c)) & 0xffu : b;
            }
            tile[(kOwnRows * wave + i) * (3 * kTileW) + 3 * col + c] = (uint8_t)b;
        }
    __syncthreads();

    const int ly = t / kLanesX, lx = t - ly * kLanesX;
    const int x = px0 + kRun * lx;
    const int npix = min(kRun, a.out_w - x);
    if (npix <= 0) return;
#pragma unroll
    for (int u = ly; u < kTileH; u += kRowStep) {
        const int y = py0 + u;
        if (y >= a.out_h) break;
        const uint32_t *run = reinterpret_cast<const uint32_t *>(tile + u * (3 * kTileW) + 3 * kRun * lx);
        const uint32_t w[3] = {run[0], run[1], run[2]};
        uint32_t o[kRun][3];
#pragma unroll
        for (int k = 0; k < kRun; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) o[k][c] = (w[(3 * k + c) >> 2] >> (8 * ((3 * k + c) & 3))) & 0xffu;
        sink(o, y, x, npix);
    }
}

}  // namespace jpeg_amd
