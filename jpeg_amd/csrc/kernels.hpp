// kernels.hpp -- internal launch interface between the C ABI (capi.hip) and the gfx950
// kernels (kernels_*.hip).  Everything here is device-resident and asynchronous on `stream`.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/jpeg_amd.h"
#include "huffman_interval.hpp"

namespace jpeg_amd {

// Streaming output (written once, never re-read by the launch chain): the `nt` hint keeps it
// from displacing data that IS re-read (chroma intermediates, tables) in L2 and the Infinity
// Cache.  Only for instructions that write WHOLE 128-byte lines: on accesses that touch a line
// 16 bytes at a time (one block per work-item loads / stores) `nt` defeats the merging of the
// pieces and halves the throughput (measured: IDCT-only 184 -> 351 us, encode 38 -> 71 us).
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_nt16(void *p, const uint4 &v)
{
    __builtin_nontemporal_store(u32x4_t{v.x, v.y, v.z, v.w}, reinterpret_cast<u32x4_t *>(p));
}

// Per-plane description of a batch of identically laid out images.
// image i of plane p lives at ptr[p] + i * stride[p] (elements).
struct PlaneSet {
    const void *ptr[JPEG_AMD_MAX_PLANES];
    size_t      stride[JPEG_AMD_MAX_PLANES];
};
struct PlaneSetMut {
    void  *ptr[JPEG_AMD_MAX_PLANES];
    size_t stride[JPEG_AMD_MAX_PLANES];
};

// Quantisation tables in HBM: uint16 [n_images or 1][ntables][64] zigzag.
struct QuantaRef {
    const uint16_t *d_quanta;
    size_t          image_stride;  // uint16 elements between image table sets (0 = shared)
};

enum class PixelKind : int { Rect16 = 0, YCC8 = 1, RGB8 = 2 };

// ---- decode -------------------------------------------------------------------------
// a3..a7: dequantise + IDCT of one plane (batch of n_images), output uint16 or uint8 samples.
hipError_t launch_idct_plane(hipStream_t stream, int n_images, const int16_t *d_coef,
                             size_t coef_stride, QuantaRef q, int qi, int ux, int uy,
                             int precision, void *d_plane, size_t plane_stride,
                             bool out_u8);

// Sparse coefficients (entropy.cpp, jpeg_amd_jpeg_decode_sparse) -> the planes.  d_skip: optional per-image flags, nonzero =
// leave that image's planes alone.  d_packed (optional): the images' records [descriptors][entries] lie packed in d_desc, image i's
// at element d_packed[i] (the strides and d_entries are then not used).
hipError_t launch_expand_sparse(hipStream_t stream, int n_images, const jpeg_amd_layout &layout, const uint32_t *d_desc,
                                size_t desc_stride, const uint32_t *d_entries, size_t entries_stride, const uint8_t *d_skip,
                                const PlaneSetMut &coef, const uint64_t *d_packed = nullptr);

// ... and the planes -> sparse coefficients (for jpeg_amd_jpeg_encode_sparse).  d_cursor: one uint32 per image, on return the
// number of entries the image has; larger than `capacity`: the image did not fit and its entries are not valid.
hipError_t launch_sparsify(hipStream_t stream, int n_images, const jpeg_amd_layout &layout, const PlaneSet &coef, uint32_t *d_desc,
                           size_t desc_stride, uint32_t *d_entries, size_t entries_stride, uint32_t capacity, uint32_t *d_cursor);

// ---- windowed, mixed-geometry expand (kernels_expand.hip) ------------------------------------------------
// launch_expand_sparse for images of different geometries in ONE launch of nwg workgroups (k_expand_mixed), each plane cut
// to a window of blocks and each block to its first `head` octets: what include/jpeg_amd.h ("files to tensors") says of
// jpeg_amd_spectral_expand_mixed.  d_items: one record of expand_mixed_record_bytes() bytes per image, 16-byte aligned,
// written by expand_mixed_record on the host from an item that is VALID (windows inside their planes, head 1 | 4 | 8);
// d_groups: uint32 [n_images + 1], the prefix of expand_mixed_groups over the images (d_groups[n_images] == nwg, at most
// 2^31 - 1); d_records: what the items' desc_at and entries_at count from.
size_t     expand_mixed_record_bytes();
uint64_t   expand_mixed_groups(const jpeg_amd_expand_item &item);   // workgroups of one image
void       expand_mixed_record(void *dst, const jpeg_amd_expand_item &item);
hipError_t launch_expand_mixed(hipStream_t stream, int n_images, const void *d_items, const uint32_t *d_groups, uint32_t nwg,
                               const uint32_t *d_records);

// ---- entropy decoding on the device (kernels_entropy.hip) -----------------------------------------------
// One launch of k_huffman_intervals: a work-item per restart interval.  `base`: a buffer in device memory, 16-byte aligned,
// of base_bytes bytes, that holds the files' blocks (interval_plan.hpp); `files`: a record per file, with its whole planes
// (16-byte aligned) and where its block lies behind `base`; first[f]: the intervals of the files before f, first[nfiles] ==
// nwork, the launch's work-items; status: one word per interval, in that order.  The host has checked every interval
// (interval_plan.hpp, work_fits); the kernel checks what it takes from device memory once more.
struct IntervalLaunch {
    const uint8_t *base;
    const interval::IntervalFile *files;
    const uint32_t *first;
    int32_t *status;
    uint64_t base_bytes;
    uint32_t nfiles, nwork;
};
hipError_t launch_huffman_intervals(hipStream_t stream, const IntervalLaunch &launch);

// a9 (+ a11/a12): upsample + interleave, written as Rectangular uint16, or colour-converted
// straight to YCbCr / RGB bytes.  Planes are uint16 (or uint8 when planes_u8).
hipError_t launch_planar_to_pixels(hipStream_t stream, int n_images,
                                   const jpeg_amd_layout &layout, const PlaneSet &planes,
                                   bool planes_u8, bool cosited, PixelKind kind,
                                   void *d_out, size_t out_stride_bytes);

// ... and back: Rectangular -> Spectral in one launch (decomposed() + fdct(quanta:), encode.swift:389-425, 199-248), same layouts.
bool       generic_encode_supported(const jpeg_amd_layout &layout);
hipError_t launch_generic_encode(hipStream_t stream, int n_images, const jpeg_amd_layout &layout, const uint16_t *d_rect,
                                 size_t rect_stride, QuantaRef q, const PlaneSetMut &coef);

// a10..a12: Rectangular.unpack(as:) for YCbCr / RGB.
hipError_t launch_unpack(hipStream_t stream, const uint16_t *d_rect, size_t npixels,
                         int nplanes, jpeg_amd_color color, uint8_t *d_pixels);

// Fused Spectral -> YCbCr / RGB bytes (kernels_fused.hip): 8-bit y8 images, and ycc8 images
// with full-factor luma and 1x / 2x subsampled chroma, centred upsampling.
bool       fused_decode_supported(const jpeg_amd_layout &layout, bool cosited);
// No intermediate in HBM for any layout.  `d_walk_counters`: a device dword that the caller keeps for the stream
// (jpeg_amd_ctx owns one): the 4:2:0 walk of a long call hands its stacks out through it (zeroed in front of the launch,
// on the stream); nullptr: always the static walk.
hipError_t launch_fused_decode(hipStream_t stream, int n_images, const jpeg_amd_layout &layout,
                               const PlaneSet &coef, QuantaRef q, bool rgb, uint32_t *d_walk_counters,
                               uint8_t *d_pixels, size_t pixel_stride);

// ycc8 4:2:0 in ONE launch with no chroma intermediate in HBM (kernels_quad.hip): the waves of a workgroup decode a
// stack of vertically adjacent strips together and share one chroma tile in LDS.  Any image size; launch_fused_decode
// sends every 4:2:0 call here.
bool       quad_decode_supported(const jpeg_amd_layout &layout);
hipError_t launch_quad_decode(hipStream_t stream, int n_images, const jpeg_amd_layout &layout,
                              const PlaneSet &coef, QuantaRef q, bool rgb, uint32_t *d_walk_counters,
                              uint8_t *d_pixels, size_t pixel_stride);

// Spectral -> Rectangular (uint16 [H][W][count]) in one launch for the JPEG.Format plug-in path (kernels_generic.hip): any
// precision 1 .. 16, 1 .. 4 planes, centred or cosited, every plane at the image's scale or at half of it per axis.
bool       generic_fused_supported(const jpeg_amd_layout &layout);
// `d_walk_counter`: TWO device dwords the caller keeps for the stream, zero when handed over (calls of several rounds draw their tiles
// through them and leave them zero; nullptr: planned)
hipError_t launch_generic_fused(hipStream_t stream, int n_images, const jpeg_amd_layout &layout, const PlaneSet &coef,
                                QuantaRef q, bool cosited, uint32_t *d_walk_counter, uint16_t *d_rect, size_t rect_stride);

// ---- tile decode (kernels_tile.hip) ------------------------------------------------------
// The layouts of fused_decode_supported, n x n samples per block (n = 8 / denom): ONE launch of one of the four kernels whose
// workgroup decodes a tile of output pixels straight from the coefficients.  What the host stages for the rectangle grids --
// per image of the call a rectangle or a record, per launch an index list and a tile prefix -- is tile_staging.hpp's, which
// also holds the tile count (rect_tiles) and the tile heights.
enum class TileKernel : int {
    Region,   // k_region_decode: n = 8; image i of the launch is image i of the call, cut to its rectangle; tiles of kRegionTileH rows
    Scaled,   // k_scaled_decode: n in {4, 2, 1}; whole scaled images of width x height on a static grid, nothing staged
    View,     // k_view_decode: n in {8, 4, 2, 1}; the images of a call that share n, each cut to its rectangle of the scaled image
    Mixed,    // k_view_decode_mixed: View for images of different layouts that share n and the number of planes (1 or 3)
};
struct TileLaunch {
    TileKernel kernel;
    int  n, nplanes;
    bool rgb;
    // The images -- Region, Scaled, View: `layout` is the FULL-SIZE image's (nplanes its number of planes); image i's
    // coefficients, tables and pixels (rows of its width * 3 bytes, unpadded, at d_pixels + i * pixel_stride) are image i of
    // the CALL's.  Mixed: all of that is in the image's record.
    const jpeg_amd_layout *layout;
    PlaneSet  coef;
    QuantaRef q;
    uint8_t  *d_pixels;
    size_t    pixel_stride;
    int       width, height;   // Scaled: W', H'
    int       n_images;        // of the launch
    // What is staged -- Region, View, Mixed: the words of a TileStaging on the device.  d_payload: word 0, 16-byte aligned
    // (Region, View: the rectangles of rect(); Mixed: records of mixed_record_bytes() bytes, written by mixed_record);
    // d_index, d_tiles, nwg: the launch's TileGroup in them, over rect_tiles(n, kRegionTileH or kViewTileH, rectangle).
    // Region does not read d_index.
    const void     *d_payload;
    const uint32_t *d_index, *d_tiles;
    uint32_t        nwg;
};
// Nothing is launched for no images or no workgroups.  hipErrorInvalidValue: an n that `kernel` is not built for, planes other
// than 1 or 3, or (Region, Scaled, View) no layout or one of another number of planes.
hipError_t launch_tile_decode(hipStream_t stream, const TileLaunch &launch);

// A record of the Mixed kernel: `layout` is one of fused_decode_supported, `region` a rectangle of its image at n samples per
// block, d_pixels where that rectangle's first pixel goes (rows of region.width * 3 bytes).
size_t     mixed_record_bytes();
void       mixed_record(void *dst, const jpeg_amd_layout &layout, int n, const int16_t *const d_coef[], const uint16_t *d_quanta,
                        const jpeg_amd_region &region, uint8_t *d_pixels);

// The fallbacks of the layouts without a tile kernel.  Any layout: whole decoded images (width x height x 3 bytes, full_stride
// apart) cut to their rectangles (d_regions: int32 [n][4]: x, y, width, height).  max_bytes: the largest rectangle's byte count.
hipError_t launch_region_crop(hipStream_t stream, int n_images, const uint8_t *d_full, size_t full_stride, int width,
                              const int32_t *d_regions, size_t max_bytes, uint8_t *d_pixels, size_t pixel_stride);
// Any layout, n in {4, 2, 1}: one plane (ux x uy blocks) into n x n samples per block, uint16 or uint8, in a plane of
// ceil(n ux / 8) x ceil(n uy / 8) whole blocks whose padding repeats the edge samples (k_idct_scaled).
hipError_t launch_idct_scaled_plane(hipStream_t stream, int n_images, const int16_t *d_coef, size_t coef_stride, QuantaRef q,
                                    int qi, int ux, int uy, int n, int precision, void *d_plane, size_t plane_stride, bool out_u8);

// ---- resample (kernels_resample.hip) ------------------------------------------------
// n_images pixel images (rows of 3 w bytes, unpadded) resampled to out_w x out_h in ONE launch, by the contracts of
// include/jpeg_amd.h: through one of three filters ("resized decode", "antialiased resample", "bicubic resample"), read as
// stored or oriented ("oriented resample"), to bytes or to tensor elements ("tensor output").  One record per image, made on
// the host; which of the six kinds follows from the filter and from whether the call is oriented or placed.  A seventh kind,
// the WarpRecord ("warped resample"), takes the image through an affine map instead of a scale factor per axis, and an eighth,
// the ProjectRecord ("projective resample"), through a 3 x 3 homography.
struct ResizeRecord {      // bilinear
    uint64_t offset;   // bytes from d_src
    int32_t  w, h;     // > 0
    float    kx, ky;   // (float)w / (float)out_w, (float)h / (float)out_h
    uint32_t flip;     // elements out only: nonzero = the resampled image is stored mirrored along x
    uint32_t reserved;
};
// The filters with tables: antialias, the triangle widened by the scale factor, and bicubic, the Keys cubic (a = -0.5) likewise.
// Per axis the scale factor k, s = max(k, 1) and r = 1 / s.  Every kx and ky is at most kAntialiasMaxScale (bicubic:
// kBicubicMaxScale): the kernels' tables hold kAntialiasMaxTaps weights per column and row (they clamp the count to it).
struct AntialiasRecord {
    uint64_t offset;       // bytes from d_src
    int32_t  w, h;         // > 0
    float    kx, sx, rx;   // (float)w / (float)out_w, max(kx, 1.0f), 1.0f / sx
    float    ky, sy, ry;   // the same of h and out_h
    uint32_t flip;         // as ResizeRecord's
    uint32_t reserved;
};
// Oriented (orient.hpp states the eight orientations): the filter's record of the ORIENTED image -- offset the byte of its
// first pixel (OrientedSource::base), w, h and the scale factors those of the oriented extent -- and the two signed steps
// through which the walks read its pixel (x', y'); oriented_source() makes them on the host.  Every byte read lies inside the
// stored image.
struct OrientedResizeRecord : ResizeRecord {
    int64_t step_x, step_y;   // bytes from a pixel of the oriented image to its right-hand and its lower neighbour
};
struct OrientedAntialiasRecord : AntialiasRecord {
    int64_t step_x, step_y;
};
static_assert(sizeof(OrientedResizeRecord) == 48 && sizeof(OrientedAntialiasRecord) == 64, "record layout");
// Placed ("placed resample"): the oriented record of the filter -- its scale factors those of the oriented extent over the
// WINDOW's ww x wh -- and the window of the out_w x out_h canvas that the image is resampled into; the rest of the canvas is
// the launch's fill.  The window lies inside the canvas and is at least 1 x 1.
struct PlacedResizeRecord : OrientedResizeRecord {
    int32_t x0, y0, ww, wh;
};
struct PlacedAntialiasRecord : OrientedAntialiasRecord {
    int32_t x0, y0, ww, wh;
};
static_assert(sizeof(PlacedResizeRecord) == 64 && sizeof(PlacedAntialiasRecord) == 80, "record layout");
// Warped ("warped resample"): the stored image and the matrix that takes the centre of an output pixel to a point of it; there
// are no scale factors and no tables.  edge is the launch's JPEG_AMD_EDGE_* in every record of it.
struct WarpRecord {
    uint64_t offset;   // bytes from d_src
    int32_t  w, h;     // > 0, at most kWarpMaxSourceSide
    float    m[6];     // m00, m01, m02, m10, m11, m12: finite, at most kWarpMaxEntry in magnitude
    uint32_t flip;     // as ResizeRecord's
    int32_t  edge;
};
static_assert(sizeof(WarpRecord) == 48, "record layout");
// Projected ("projective resample"): the WarpRecord with the third row of the matrix, a 3 x 3 homography whose denominator the
// host has found positive and well conditioned over the whole canvas (check_project_matrix); padded to a cache-line half.
struct ProjectRecord {
    uint64_t offset;   // bytes from d_src
    int32_t  w, h;     // > 0, at most kWarpMaxSourceSide
    float    m[9];     // m00 ... m22, row by row: finite, at most kWarpMaxEntry in magnitude
    uint32_t flip;     // as ResizeRecord's
    int32_t  edge;
    uint32_t reserved;
};
static_assert(sizeof(ProjectRecord) == 64, "record layout");
// Colour ("colour stage"): beside the resample record of a tensor launch, per image the affine map of (R, G, B) that stands
// between the resample and the tensor output: row c is k[c][0 .. 2], the matrix row, and k[c][3], the offset.  The kernels read
// it once per workgroup, through uniform loads in front of the walk.
struct ColourRecord {
    float k[3][4];   // finite, at most kColourMaxEntry in magnitude
};
static_assert(sizeof(ColourRecord) == 48, "record layout");
constexpr float kColourMaxEntry = 1073741824.0f; // 2^30: three products of it with a byte and the offset stay finite
constexpr int   kWarpMaxSourceSide = 1 << 24;    // (float)w and (float)h are exact
constexpr float kWarpMaxEntry = 1073741824.0f;   // 2^30: with an output side of at most 2^30 no coordinate overflows
constexpr double kProjectMinScale = 9.31322574615478515625e-10;   // 2^-30: of S, the scale of a homography's denominator row
constexpr double kProjectMaxForeshortening = 16.0;               // S over the denominator's minimum on the canvas, at most
constexpr int   kResizeMaxSide = 1 << 30;       // of the output: the kernels' pixel indices are int
constexpr float kAntialiasMaxScale = 16.0f;
constexpr int   kAntialiasMaxTaps = 33;          // the interval [c - s, c + s] rounded outwards: 2 s + 1
constexpr float kBicubicMaxScale = 8.0f;         // "bicubic resample": [c - 2 s, c + 2 s], 4 s + 1 taps in the same tables
uint64_t   resize_tiles(int out_w, int out_h);   // workgroups per image; the launch's grid.x, which holds 2^31 - 1 at most

// Output image i at d_dst + i * dst_stride: bytes, or ELEMENTS of spec->dtype (d_dst aligned to the element), the byte of
// (image, row, flip ? out_w - 1 - x : x, channel), minus mean, times scale, converted and stored in spec->layout.  A spec is
// valid (jpeg_amd_tensor_extent).  hipErrorInvalidValue: an extent or a tile count past the limits above, null records, or a
// filter, dtype or layout that no kernel exists for.
enum class ResampleRecords : int { Stored, Oriented, Placed, Warped, Projected };   // ResizeRecord / AntialiasRecord, their Oriented*, their Placed* forms; WarpRecord (bilinear only), ProjectRecord (bilinear, or bicubic: "bicubic warp")
struct ResampleLaunch {
    int filter;                        // JPEG_AMD_FILTER_*
    ResampleRecords records;           // the kind of every record of the launch
    const jpeg_amd_tensor_spec *spec;  // nullptr: bytes out
    int n_images;
    const uint8_t *d_src;
    const void *d_records;             // record 0 of the launch; the type follows filter and records
    int out_w, out_h;
    void *d_dst;
    size_t dst_stride;
    uint8_t fill[3];                   // Placed: the bytes of a canvas pixel outside the image's window; Warped, Projected: of a tap outside the image
    // "colour stage": nullptr, or ColourRecord 0 of the launch (16-byte aligned) and the clamp's bounds, neither a NaN and
    // lo <= hi; only with a spec and with Placed, Warped or Projected records (anything else: hipErrorInvalidValue)
    const void *d_colour = nullptr;
    float lo = 0.0f, hi = 0.0f;
};
hipError_t launch_resample(hipStream_t stream, const ResampleLaunch &l);

// ---- tensors to pixel bytes (kernels_pixels.hip) ------------------------------------------------
// n_images tensors of w x h x 3 elements of source.dtype in source.layout to bytes by the contract of include/jpeg_amd.h
// ("tensor sources") in ONE launch (k_tensor_pixels).  Image i at d_src + i * src_stride ELEMENTS, d_src aligned to the
// element; its h rows of 3 w bytes at d_dst + i * dst_stride.  source is valid (jpeg_amd_tensor_source_extent).
constexpr int kTensorSourceMaxSide = 65535;      // of a source: the sides of a JPEG frame
hipError_t launch_tensor_pixels(hipStream_t stream, int n_images, const void *d_src, size_t src_stride, int w, int h,
                                const jpeg_amd_tensor_source &source, uint8_t *d_dst, size_t dst_stride);

// ---- lossless spectral transforms (kernels_transform.hip) -----------------------------
// Every plane of n_images images in one launch: output block (x, y) of plane p (out's units) reads the source block the op
// maps it to, offset by (ox[p], oy[p]) blocks (the region's origin), or zeros past in's units.  d_quanta_out: nullptr = copy,
// else requantise (q's tables -> these, same strides, plane p's table in.qi[p]).  d_overflow: optional, set to 1 where the
// reference would trap.
hipError_t launch_transform(hipStream_t stream, int n_images, int op, const jpeg_amd_layout &in, const jpeg_amd_layout &out,
                            const int *ox, const int *oy, const PlaneSet &coef_in, QuantaRef q, const uint16_t *d_quanta_out,
                            const PlaneSetMut &coef_out, int32_t *d_overflow);

// ---- spectral reduce (kernels_reduce.hip) ------------------------------------------------
// n = 8 / denom in {4, 2, 1}.  Every plane of n_images images in one launch (k_spectral_reduce): plane p of `out`
// (jpeg_amd_reduce_layout's) is Spectral.Plane.fdct of the scaled-decode samples of plane p of `in`, edge-replicated to out's
// whole blocks.  d_quanta_out: nullptr = q's tables, else the output tables (same strides, plane p's table in.qi[p]).  Every
// plane of `in` has at least one block.
hipError_t launch_spectral_reduce(hipStream_t stream, int n_images, int n, const jpeg_amd_layout &in, const jpeg_amd_layout &out,
                                  const PlaneSet &coef_in, QuantaRef q, const uint16_t *d_quanta_out, const PlaneSetMut &coef_out);

// ---- encode -------------------------------------------------------------------------
// a13: Rectangular.pack
hipError_t launch_pack(hipStream_t stream, const uint8_t *d_pixels, size_t npixels,
                       int nplanes, jpeg_amd_color color, uint16_t *d_rect);

// a14: Rectangular.decomposed() for every plane; input is Rectangular uint16, or pixel
// bytes (RGB8 / YCC8) colour-converted on the fly.
hipError_t launch_decompose(hipStream_t stream, int n_images, const jpeg_amd_layout &layout,
                            const void *d_in, size_t in_stride_bytes, PixelKind in_kind,
                            const PlaneSetMut &planes);

// Fused pixels -> Spectral (kernels_encode.hip): 8-bit y8 images, and ycc8 images with
// full-factor luma and 1x / 2x subsampled chroma.
bool       fused_encode_supported(const jpeg_amd_layout &layout);
hipError_t launch_fused_encode(hipStream_t stream, int n_images, const jpeg_amd_layout &layout,
                               const uint8_t *d_pixels, size_t pixel_stride, bool rgb, QuantaRef q,
                               const PlaneSetMut &coef);

// a15..a17: FDCT + quantise of one plane.
hipError_t launch_fdct_plane(hipStream_t stream, int n_images, const uint16_t *d_plane,
                             size_t plane_stride, QuantaRef q, int qi, int ux, int uy,
                             int precision, int16_t *d_coef, size_t coef_stride);

}  // namespace jpeg_amd
