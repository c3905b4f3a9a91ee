// kernels_resample.hip -- the resample kernels: pixel images to one target size through one of three filters, read as they are
// stored or in one of the eight EXIF orientations, to bytes or to normalised tensor elements.  The contracts are in
// include/jpeg_amd.h ("resized decode", "antialiased resample", "bicubic resample", "oriented resample", "tensor output"); the
// walks, the filters and the stores are resample.hpp's, antialias.hpp's, mapped_walk.hpp's and tensor_sink.hpp's.  Filter,
// record kind and sink are three parameters; a kernel is a walk with a sink:
//
// k_resize_bilinear: bilinear, stored, bytes -- resample_walk written out with the packing inside the tap loop (below).
// k_resize_oriented_bytes: bilinear, oriented, bytes -- resample_walk<true> with byte_sink.
// k_resize_tensor<Oriented, T, CHW>: bilinear, elements of T in either layout -- resample_walk<Oriented> with tensor_sink.
// k_tables_bytes<Filter, Record>, k_tables_tensor<Filter, Record, T, CHW>: the filters with weight tables (TriangleFilter:
//   antialias, BicubicFilter) over AntialiasRecords or OrientedAntialiasRecords -- antialias_walk with the same two sinks.
// k_resize_placed_bytes, k_resize_placed_tensor<T, CHW>, k_tables_placed_bytes<Filter>, k_tables_placed_tensor<Filter, T, CHW>:
//   the same walks over PlacedResizeRecords / PlacedAntialiasRecords ("placed resample") with the same sinks; their arguments
//   end with the launch's fill.
// k_mapped_bytes<Map, Taps>, k_mapped_tensor<Map, Taps, Colour, T, CHW>: mapped_walk (mapped_walk.hpp) with the same two sinks and
//   the placed kernels' arguments; no tables, no LDS.  AffineMap over WarpRecords with TwoTaps is "warped resample";
//   ProjectiveMap over ProjectRecords is "projective resample" with TwoTaps and "bicubic warp" with CubicTaps.
// k_resize_placed_tensor, k_tables_placed_tensor and k_mapped_tensor carry a Colour flag: with it the sink is colour_sink
//   ("colour stage": an affine map of (R, G, B) per image and a clamp, in front of the mean), the arguments end with the
//   ColourRecords and the clamp's bounds, and nothing else differs (walk_to_tensor).  These three express every record kind
//   -- a whole-canvas window is the oriented and the stored call -- so the others have no colour form.
// The byte kernels never flip (the records' flip is not read); the tensor kernels flip where the record says so, after the
// orientation: the flip mirrors the OUTPUT columns.
//
// Reads stay inside the stored image: the walks clamp, and an oriented pixel (x', y') of the oriented extent is a stored
// pixel.  With a transposing orientation (5 .. 8) neighbouring lanes read bytes a stored row apart instead of 3 bytes apart:
// more cache lines per load, the same lines per tile.  Writes stay inside out_h rows of 3 out_w bytes, or 3 out_w out_h
// elements, of the image's slot.  LDS as the walks' (tables: 38 016 bytes).
//
// Compile with -ffp-contract=off (see dct.hpp).
#pragma clang fp contract(off)

#include <type_traits>

#include "antialias.hpp"
#include "fused_common.hpp"
#include "kernels.hpp"
#include "mapped_walk.hpp"
#include "resample.hpp"
#include "tensor_sink.hpp"

namespace jpeg_amd {

namespace {

struct ResizeArgs : ResampleArgs {   // k_resize_bilinear's
    uint8_t *dst;
    size_t dst_stride;   // bytes between output images
};

// Every other kernel's arguments, one struct per sink.  tab_records: the records of the kernels with tables, which do not read
// ResampleArgs::records (that slot stays where it is: taking it out moves every scalar load); the oriented bilinear kernels
// read ResampleArgs::records and leave this one alone.
template <typename Record>
struct BytesArgs : ResampleArgs {
    const Record *tab_records;
    uint8_t *dst;
    size_t dst_stride;   // bytes between output images
};

template <typename T, typename Record>
struct RecordTensorArgs : TensorArgs<T> {
    const Record *tab_records;
};

// The placed kernels': the oriented kernels' of the sink, then the fill, channel c in bits 8 c ...
template <typename Record>
struct PlacedBytesArgs : BytesArgs<Record> {
    uint32_t fill;
};
template <typename T, typename Record>
struct PlacedTensorArgs : RecordTensorArgs<T, Record> {
    uint32_t fill;
};
// ... and with the "colour stage": the placed tensor kernels' (the warp's are those), then the records and the clamp.
template <typename T, typename Record>
struct ColourTensorArgs : PlacedTensorArgs<T, Record> {
    const ColourRecord *colour;
    float lo, hi;
};
template <bool Colour, typename T, typename Record>
using PlacedSinkArgs = typename std::conditional<Colour, ColourTensorArgs<T, Record>, PlacedTensorArgs<T, Record>>::type;

// Where the image of the workgroup goes, and the elements of one of its channels in CHW.
template <typename Args>
__device__ __forceinline__ auto image_dst(const Args &a) { return a.dst + (size_t)blockIdx.y * a.dst_stride; }
__device__ __forceinline__ size_t image_plane(const ResampleArgs &a) { return (size_t)(uint32_t)a.out_w * (uint32_t)a.out_h; }

// The byte sink of every kernel but k_resize_bilinear: the 12 bytes of a run packed into three dwords and stored as that kernel
// does (store_run).
__device__ __forceinline__ void byte_sink(uint8_t *dst, int out_w, const uint32_t (&o)[kRun][3], int y, int x, int npix)
{
    uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < kRun; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) w[(3 * k + c) >> 2] |= o[k][c] << (8 * ((3 * k + c) & 3));
    store_run(dst + 3 * ((size_t)(uint32_t)y * (uint32_t)out_w + (uint32_t)x), w[0], w[1], w[2], 3 * npix);
}

// The walk that resample.hpp describes (resample_walk, never flipped), written out here with the packing inside the tap loop.
// Through resample_walk, which hands over a finished run, the compiler packs the 12 bytes with four instructions per dword
// where this text gets three, and the kernel measured 1.3 % slower on the MI355X (profiles/resample_refactor.txt); so this
// kernel keeps its own text, and a change to the walk is made in both places.  Where 3 out_w, dst_stride and d_dst are
// multiples of 4 -- 224 x 224 into a dense tensor -- every full run is three dword stores.
__global__ __launch_bounds__(kThreads) void k_resize_bilinear(ResizeArgs a)
{
    __shared__ int cx0[kTileW], cx1[kTileW], ry0[kTileH], ry1[kTileH];
    __shared__ float cfx[kTileW], rfy[kTileH];

    const int t = threadIdx.x;
    uint32_t txi;
    const uint32_t tyi = a.tiles_x.div(blockIdx.x, txi);
    const int px0 = kTileW * (int)txi, py0 = kTileH * (int)tyi;
    const ResizeRecord r = a.records[blockIdx.y];
    if (t < kTileW) {
        int i0 = 0, i1 = 0;
        float f = 0.0f;
        if (px0 + t < a.out_w) axis_tap(px0 + t, r.kx, r.w, i0, i1, f);
        cx0[t] = i0; cx1[t] = i1; cfx[t] = f;
    } else if (t < kTileW + kTileH) {
        const int u = t - kTileW;
        int i0 = 0, i1 = 0;
        float f = 0.0f;
        if (py0 + u < a.out_h) axis_tap(py0 + u, r.ky, r.h, i0, i1, f);
        ry0[u] = i0; ry1[u] = i1; rfy[u] = f;
    }
    __syncthreads();

    const int ly = t / kLanesX, lx = t - ly * kLanesX;
    const int x = px0 + kRun * lx;
    const int npix = min(kRun, a.out_w - x);
    if (npix <= 0) return;
    size_t x0[kRun], x1[kRun];
    float fx[kRun];
#pragma unroll
    for (int k = 0; k < kRun; ++k) {
        x0[k] = (size_t)3 * (uint32_t)cx0[kRun * lx + k];
        x1[k] = (size_t)3 * (uint32_t)cx1[kRun * lx + k];
        fx[k] = cfx[kRun * lx + k];
    }
    const size_t row_bytes = (size_t)3 * (uint32_t)r.w;
    const uint8_t *src = a.src + r.offset;
    uint8_t *dst = a.dst + (size_t)blockIdx.y * a.dst_stride;
#pragma unroll
    for (int u = ly; u < kTileH; u += kRowStep) {
        const int y = py0 + u;
        if (y >= a.out_h) break;
        const uint8_t *r0 = src + (size_t)(uint32_t)ry0[u] * row_bytes, *r1 = src + (size_t)(uint32_t)ry1[u] * row_bytes;
        const float fy = rfy[u];
        uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < kRun; ++k) {
            const uint8_t *pa = r0 + x0[k], *pb = r0 + x1[k], *pc = r1 + x0[k], *pd = r1 + x1[k];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t o = resample((float)pa[c], (float)pb[c], (float)pc[c], (float)pd[c], fx[k], fy);
                w[(3 * k + c) >> 2] |= o << (8 * ((3 * k + c) & 3));
            }
        }
        store_run(dst + 3 * ((size_t)(uint32_t)y * (uint32_t)a.out_w + (uint32_t)x), w[0], w[1], w[2], 3 * npix);
    }
}

__global__ __launch_bounds__(kThreads) void k_resize_oriented_bytes(BytesArgs<OrientedResizeRecord> a)
{
    uint8_t *dst = image_dst(a);
    resample_walk<true>(a, false, [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) { byte_sink(dst, a.out_w, o, y, x, npix); });
}

template <bool Oriented, typename T>
using ResizeTensorArgs = typename std::conditional<Oriented, RecordTensorArgs<T, OrientedResizeRecord>, TensorArgs<T>>::type;

// The stored records' instantiations keep the text of tensor_sink in their body, as they did when they were the only ones:
// handed the function, four of the six compile to other code (fewer instructions, another schedule), and the bilinear kernels
// are to stay the code they were until that form has been timed.
template <bool Oriented, typename T, bool CHW>
__global__ __launch_bounds__(kThreads) void k_resize_tensor(ResizeTensorArgs<Oriented, T> a)
{
    T *dst = image_dst(a);
    const size_t plane = image_plane(a);
    resample_walk<Oriented>(a, true, [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) {
        if constexpr (Oriented) {
            tensor_sink<T, CHW>(a, dst, plane, o, y, x, npix);
        } else {
            T e[CHW ? 3 : 1][CHW ? kRun : 3 * kRun];   // CHW: three runs of kRun, HWC: one run of 3 kRun
#pragma unroll
            for (int k = 0; k < kRun; ++k) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float d = (float)o[k][c] - a.mean[c];
                    e[CHW ? c : 0][CHW ? k : 3 * k + c] = to_element<T>(d * a.scale[c]);
                }
            }
            const size_t at = (size_t)(uint32_t)y * (uint32_t)a.out_w + (uint32_t)x;
            if constexpr (CHW) {
#pragma unroll
                for (int c = 0; c < 3; ++c) store_elems<T, kRun>(dst + c * plane + at, e[c], npix);
            } else {
                store_elems<T, 3 * kRun>(dst + 3 * at, e[0], 3 * npix);
            }
        }
    });
}

template <typename Filter, typename Record>
__global__ __launch_bounds__(kThreads) void k_tables_bytes(BytesArgs<Record> a)
{
    uint8_t *dst = image_dst(a);
    antialias_walk<Filter>(a, a.tab_records, false, [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) { byte_sink(dst, a.out_w, o, y, x, npix); });
}

template <typename Filter, typename Record, typename T, bool CHW>
__global__ __launch_bounds__(kThreads) void k_tables_tensor(RecordTensorArgs<T, Record> a)
{
    T *dst = image_dst(a);
    const size_t plane = image_plane(a);
    antialias_walk<Filter>(a, a.tab_records, true, [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) {
        tensor_sink<T, CHW>(a, dst, plane, o, y, x, npix);
    });
}

__global__ __launch_bounds__(kThreads) void k_resize_placed_bytes(PlacedBytesArgs<PlacedResizeRecord> a)
{
    uint8_t *dst = image_dst(a);
    resample_walk<true, true>(a, false, [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) { byte_sink(dst, a.out_w, o, y, x, npix); }, a.fill);
}

// walk(sink) with the sink of a tensor kernel that carries a Colour flag.  Colour: the image's ColourRecord, read here, once
// per workgroup and in front of the walk, and colour_sink in tensor_sink's place.  Handed the walk as a generic lambda, all
// kernels are the instructions they were when each spelled this block out, but for the three bicubic k_mapped_tensor<...,
// false, T, true>: one address computation in front of their row loop stands two instructions later (measured:
// profiles/mapped_walk_refactor.txt).
template <bool Colour, typename T, bool CHW, typename Args, typename Walk>
__device__ __forceinline__ void walk_to_tensor(const Args &a, Walk walk)
{
    T *dst = image_dst(a);
    const size_t plane = image_plane(a);
    if constexpr (Colour) {
        const ColourRecord k = a.colour[blockIdx.y];
        walk([&](const uint32_t (&o)[kRun][3], int y, int x, int npix) { colour_sink<T, CHW>(a, k, a.lo, a.hi, dst, plane, o, y, x, npix); });
    } else {
        walk([&](const uint32_t (&o)[kRun][3], int y, int x, int npix) { tensor_sink<T, CHW>(a, dst, plane, o, y, x, npix); });
    }
}

template <bool Colour, typename T, bool CHW>
__global__ __launch_bounds__(kThreads) void k_resize_placed_tensor(PlacedSinkArgs<Colour, T, PlacedResizeRecord> a)
{
    walk_to_tensor<Colour, T, CHW>(a, [&](auto sink) { resample_walk<true, true>(a, true, sink, a.fill); });
}

template <typename Filter>
__global__ __launch_bounds__(kThreads) void k_tables_placed_bytes(PlacedBytesArgs<PlacedAntialiasRecord> a)
{
    uint8_t *dst = image_dst(a);
    antialias_walk<Filter>(a, a.tab_records, false, [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) { byte_sink(dst, a.out_w, o, y, x, npix); }, a.fill);
}

template <bool Colour, typename Filter, typename T, bool CHW>
__global__ __launch_bounds__(kThreads) void k_tables_placed_tensor(PlacedSinkArgs<Colour, T, PlacedAntialiasRecord> a)
{
    walk_to_tensor<Colour, T, CHW>(a, [&](auto sink) { antialias_walk<Filter>(a, a.tab_records, true, sink, a.fill); });
}

template <typename Map, typename Taps>
__global__ __launch_bounds__(kThreads) void k_mapped_bytes(PlacedBytesArgs<typename Map::Record> a)
{
    uint8_t *dst = image_dst(a);
    mapped_walk<Map, Taps>(a, a.tab_records, false, a.fill, [&](const uint32_t (&o)[kRun][3], int y, int x, int npix) { byte_sink(dst, a.out_w, o, y, x, npix); });
}

template <typename Map, typename Taps, bool Colour, typename T, bool CHW>
__global__ __launch_bounds__(kThreads) void k_mapped_tensor(PlacedSinkArgs<Colour, T, typename Map::Record> a)
{
    walk_to_tensor<Colour, T, CHW>(a, [&](auto sink) { mapped_walk<Map, Taps>(a, a.tab_records, true, a.fill, sink); });
}

// ---- the launcher ----

// f(T{}, std::bool_constant<CHW>{}) for the element type and the layout of spec, or what no kernel exists for.
template <typename F>
hipError_t with_element(const jpeg_amd_tensor_spec &spec, F f)
{
    const bool chw = spec.layout == JPEG_AMD_TENSOR_CHW;
    if (!chw && spec.layout != JPEG_AMD_TENSOR_HWC) return hipErrorInvalidValue;
    const auto in_layout = [&](auto t) { return chw ? f(t, std::true_type{}) : f(t, std::false_type{}); };
    switch (spec.dtype) {
    case JPEG_AMD_F32: return in_layout(float{});
    case JPEG_AMD_F16: return in_layout(_Float16{});
    case JPEG_AMD_BF16: return in_layout(bf16_t{});
    default: return hipErrorInvalidValue;
    }
}

// The "colour stage" of the launch into the args that have one.
template <typename Args>
void set_colour(Args &, const ResampleLaunch &) {}
template <typename T, typename Record>
void set_colour(ColourTensorArgs<T, Record> &a, const ResampleLaunch &l)
{
    a.colour = static_cast<const ColourRecord *>(l.d_colour);
    a.lo = l.lo;
    a.hi = l.hi;
}

// The args of a kernel, zeroed.
template <typename Args>
Args kernel_args(void (*)(Args)) { return Args{}; }

struct Bilinear;   // in place of a filter of antialias.hpp: resample_walk, whose records are ResampleArgs::records

// The launch of one filter and record kind: `run` fills the args of a kernel, whatever its sink, the rest names the kernel.
template <typename Filter, typename Record>
hipError_t launch_kernel(hipStream_t stream, const ResampleLaunch &l, const ResampleArgs &head, dim3 grid)
{
    constexpr bool projected = std::is_same<Record, ProjectRecord>::value;
    constexpr bool warped = std::is_same<Record, WarpRecord>::value || projected;   // (mapped_walk; the placed kernels' args: records in tab_records, a fill)
    constexpr bool bilinear = std::is_same<Filter, Bilinear>::value, oriented = std::is_same<Record, OrientedResizeRecord>::value;
    constexpr bool placed = std::is_same<Record, PlacedResizeRecord>::value || std::is_same<Record, PlacedAntialiasRecord>::value;
    constexpr bool cubic = projected && !bilinear;   // "bicubic warp": BicubicFilter names the filter, the taps are CubicTaps
    using Map = typename std::conditional<projected, ProjectiveMap, AffineMap>::type;   // (warped: mapped_walk's map and taps)
    using Taps = typename std::conditional<cubic, CubicTaps, TwoTaps>::type;
    const auto run = [&](auto kernel) {
        auto a = kernel_args(kernel);
        static_cast<ResampleArgs &>(a) = head;
        if constexpr (bilinear && !warped)
            a.records = static_cast<const Record *>(l.d_records);
        else
            a.tab_records = static_cast<const Record *>(l.d_records);
        a.dst = static_cast<decltype(a.dst)>(l.d_dst);
        a.dst_stride = l.dst_stride;
        if constexpr (placed || warped) a.fill = (uint32_t)l.fill[0] | (uint32_t)l.fill[1] << 8 | (uint32_t)l.fill[2] << 16;
        set_colour(a, l);
        if constexpr (!std::is_same<decltype(a.dst), uint8_t *>::value) {
            for (int c = 0; c < 3; ++c) {
                a.mean[c] = l.spec->mean[c];
                a.scale[c] = l.spec->scale[c];
            }
        }
        hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, a);
        return hipGetLastError();
    };
    // The kernel with the tensor sink for elements of t in the layout chw; colour: with the "colour stage", where there is one.
    const auto tensor_kernel = [](auto colour, auto t, auto chw) {
        using T = decltype(t);
        constexpr bool Colour = decltype(colour)::value, CHW = decltype(chw)::value;
        if constexpr (warped)
            return k_mapped_tensor<Map, Taps, Colour, T, CHW>;
        else if constexpr (placed && bilinear)
            return k_resize_placed_tensor<Colour, T, CHW>;
        else if constexpr (placed)
            return k_tables_placed_tensor<Colour, Filter, T, CHW>;
        else if constexpr (bilinear)
            return k_resize_tensor<oriented, T, CHW>;
        else
            return k_tables_tensor<Filter, Record, T, CHW>;
    };
    if (l.d_colour && !(l.spec && (placed || warped))) return hipErrorInvalidValue;   // "colour stage": these kernels only
    if (l.spec) {
        return with_element(*l.spec, [&](auto t, auto chw) {
            if constexpr (placed || warped) {
                if (l.d_colour) return run(tensor_kernel(std::true_type{}, t, chw));
            }
            return run(tensor_kernel(std::false_type{}, t, chw));
        });
    }
    if constexpr (warped)
        return run(k_mapped_bytes<Map, Taps>);
    else if constexpr (placed && bilinear)
        return run(k_resize_placed_bytes);
    else if constexpr (placed)
        return run(k_tables_placed_bytes<Filter>);
    else if constexpr (!bilinear)
        return run(k_tables_bytes<Filter, Record>);
    else if constexpr (oriented)
        return run(k_resize_oriented_bytes);
    else
        return run(k_resize_bilinear);
}

template <typename Filter, typename Stored, typename Oriented, typename Placed>
hipError_t launch_filter(hipStream_t stream, const ResampleLaunch &l, const ResampleArgs &head, dim3 grid)
{
    switch (l.records) {
    case ResampleRecords::Stored: return launch_kernel<Filter, Stored>(stream, l, head, grid);
    case ResampleRecords::Oriented: return launch_kernel<Filter, Oriented>(stream, l, head, grid);
    case ResampleRecords::Placed: return launch_kernel<Filter, Placed>(stream, l, head, grid);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

uint64_t resize_tiles(int out_w, int out_h)
{
    return (uint64_t)((out_w + kTileW - 1) / kTileW) * (uint64_t)((out_h + kTileH - 1) / kTileH);
}

hipError_t launch_resample(hipStream_t stream, const ResampleLaunch &l)
{
    if (l.n_images == 0) return hipSuccess;
    if (!l.d_records) return hipErrorInvalidValue;
    ResampleArgs head{};
    dim3 grid;
    if (const hipError_t e = resample_launch(l.n_images, l.d_src, nullptr, l.out_w, l.out_h, head, grid)) return e;
    if (l.records == ResampleRecords::Warped)   // "warped resample": the two-tap filter only
        return l.filter == JPEG_AMD_FILTER_BILINEAR ? launch_kernel<Bilinear, WarpRecord>(stream, l, head, grid) : hipErrorInvalidValue;
    if (l.records == ResampleRecords::Projected) {   // "projective resample", or "bicubic warp" over the same records
        if (l.filter == JPEG_AMD_FILTER_BICUBIC) return launch_kernel<BicubicFilter, ProjectRecord>(stream, l, head, grid);
        return l.filter == JPEG_AMD_FILTER_BILINEAR ? launch_kernel<Bilinear, ProjectRecord>(stream, l, head, grid) : hipErrorInvalidValue;
    }
    switch (l.filter) {
    case JPEG_AMD_FILTER_BILINEAR: return launch_filter<Bilinear, ResizeRecord, OrientedResizeRecord, PlacedResizeRecord>(stream, l, head, grid);
    case JPEG_AMD_FILTER_ANTIALIAS: return launch_filter<TriangleFilter, AntialiasRecord, OrientedAntialiasRecord, PlacedAntialiasRecord>(stream, l, head, grid);
    case JPEG_AMD_FILTER_BICUBIC: return launch_filter<BicubicFilter, AntialiasRecord, OrientedAntialiasRecord, PlacedAntialiasRecord>(stream, l, head, grid);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace jpeg_amd
