/* jpeg_amd.h -- C ABI of the MI355X (gfx950) spectral pipeline.
 *
 * Drop-in boundary for the one data-parallel hot path of tayloraswift/jpeg
 * (reference @ 2024_08_07; citations below are sources/jpeg/<file>:<lines>):
 *
 *   decode   Spectral.idct()              decode.swift:4154-4165  (per plane :4101-4133)
 *            Planar.interleaved(cosite:)  decode.swift:4182-4276
 *            Rectangular.unpack(as:)      decode.swift:4291-4298  (jpeg.swift:441-453, 493-572)
 *   encode   Rectangular.pack(...)        encode.swift:453-464    (jpeg.swift:463-478, 527-599)
 *            Rectangular.decomposed()     encode.swift:389-425
 *            Planar.fdct(quanta:)         encode.swift:353-370    (per plane :199-248)
 *
 * The reference has no FFI for this path (it is pure Swift); these entry points are
 * what a Swift shim binds with @_silgen_name / a module map.
 * Results are bit-identical to the reference: the float32 operation order of the
 * reference is reproduced exactly (kernels are built with -ffp-contract=off).
 *
 * Conventions
 *   - plain C, no exceptions, no aborts: every call returns 0 (JPEG_AMD_OK) or a
 *     negative jpeg_amd_status; contract violations the reference traps on
 *     (precondition failures) come back as JPEG_AMD_EINVAL.
 *   - `d_` parameters are DEVICE pointers (HBM); `h_` parameters are HOST pointers.
 *     Quantisation tables are tiny and are HOST pointers unless named `d_`.
 *   - a ctx owns one HIP stream (or borrows the caller's), scratch memory and
 *     timing events.  A ctx is single-threaded; different ctxs may run concurrently.
 *     All device entry points are asynchronous on the ctx stream.
 *   - coefficient planes: int16 [units_y][units_x][64], ZIGZAG order inside a block
 *     (decode.swift:1434, 1466).  Spatial planes: uint16 [8*units_y][8*units_x]
 *     (decode.swift:1548-1598).  Rectangular: uint16 [H][W][nplanes]
 *     (decode.swift:1650-1718).  Colours: uint8 [H*W][3] (jpeg.swift:160-269).
 */
#ifndef JPEG_AMD_H
#define JPEG_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JPEG_AMD_VERSION 100  /* 0.1.0 */
#define JPEG_AMD_MAX_PLANES 4

typedef enum jpeg_amd_status {
    JPEG_AMD_OK      = 0,
    JPEG_AMD_EINVAL  = -1, /* bad argument / violated precondition of the reference */
    JPEG_AMD_ENOMEM  = -2, /* device or host allocation failed */
    JPEG_AMD_EHIP    = -3, /* HIP runtime error; see jpeg_amd_last_hip_error */
    JPEG_AMD_ENODEV  = -4, /* no such device / no gfx950 code object for it */
    JPEG_AMD_ENOSUP  = -5  /* valid in the reference but not implemented here */
} jpeg_amd_status;

typedef struct jpeg_amd_ctx jpeg_amd_ctx;

/* Image geometry = the part of JPEG.Layout<Format> + Spectral/Planar sizes the
 * hot path reads (jpeg.swift:1084-1635, decode.swift:2181-2190, 2456-2495).
 * Only RECOGNISED planes are listed; scale is the max sampling factor over ALL
 * components of the frame (it can exceed every listed factor). */
typedef struct jpeg_amd_layout {
    int32_t width, height;                   /* image size in pixels, > 0 */
    int32_t precision;                       /* Format.precision, 1..16 */
    int32_t nplanes;                         /* 1..JPEG_AMD_MAX_PLANES */
    int32_t scale_x, scale_y;                /* Layout.scale */
    int32_t factor_x[JPEG_AMD_MAX_PLANES];   /* Component.factor */
    int32_t factor_y[JPEG_AMD_MAX_PLANES];
    int32_t units_x[JPEG_AMD_MAX_PLANES];    /* Plane.units (data units per row / column) */
    int32_t units_y[JPEG_AMD_MAX_PLANES];
    int32_t qi[JPEG_AMD_MAX_PLANES];         /* Plane.q: index into the quanta array */
} jpeg_amd_layout;

/* colour targets of Rectangular.unpack / pack (the built-in JPEG.Color types) */
typedef enum jpeg_amd_color {
    JPEG_AMD_COLOR_YCC8 = 0,  /* JPEG.YCbCr  jpeg.swift:493-539 */
    JPEG_AMD_COLOR_RGB8 = 1   /* JPEG.RGB    jpeg.swift:551-599 */
} jpeg_amd_color;

/* ---- library / context --------------------------------------------------------- */
int         jpeg_amd_version(void);
const char *jpeg_amd_strerror(int status);
int         jpeg_amd_device_count(int *count);
/* stream: the hipStream_t to launch on (borrowed, e.g. torch's current stream; NULL is
 * the device's default stream).  With JPEG_AMD_CTX_OWN_STREAM in flags, `stream` is
 * ignored and the ctx creates (and later destroys) a private non-blocking stream. */
#define JPEG_AMD_CTX_OWN_STREAM 1
/* With JPEG_AMD_CTX_DEVICE_ENTROPY in flags, the batch file calls (jpeg_amd_decompress_batch, _batch_device and every
 * jpeg_amd_decompress_*_mixed call) ask jpeg_amd_jpeg_plan_intervals about each file first: a file it takes, whose
 * entropy-coded bytes, tables and interval list fit the staging of its coefficient planes (of its first plane in the calls of
 * one geometry; about 6 kB of that are Huffman tables, so images of a few blocks stay on the host), is uploaded as
 * those bytes and Huffman-decoded on the device (k_huffman_intervals) in front of the chunk's other kernels; every other file
 * takes the host route in the same chunk.  Results are the same either way.  A device file whose status is not OK ends the call
 * with that status, as a file that proves damaged after the call has started does.  jpeg_amd_decompress (one file) and
 * jpeg_amd_decompress_rectangular decode on the host whatever the flag says. */
#define JPEG_AMD_CTX_DEVICE_ENTROPY 2
int         jpeg_amd_ctx_create(int device, void *stream, int flags, jpeg_amd_ctx **ctx);
int         jpeg_amd_ctx_destroy(jpeg_amd_ctx *ctx);
int         jpeg_amd_ctx_synchronize(jpeg_amd_ctx *ctx);
int         jpeg_amd_last_hip_error(const jpeg_amd_ctx *ctx); /* raw hipError_t */
/* fill in units_x/units_y = ceil(size * factor / (8 * scale))  decode.swift:2606-2616 */
int         jpeg_amd_layout_units(jpeg_amd_layout *layout);

/* ---- device memory + timing (so a non-HIP host language can keep data resident) -- */
int jpeg_amd_malloc(jpeg_amd_ctx *ctx, size_t bytes, void **d_ptr);
int jpeg_amd_free(jpeg_amd_ctx *ctx, void *d_ptr);
int jpeg_amd_memcpy_h2d(jpeg_amd_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int jpeg_amd_memcpy_d2h(jpeg_amd_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
/* HIP events on the ctx stream; end() synchronises and returns elapsed ms */
int jpeg_amd_timer_begin(jpeg_amd_ctx *ctx);
int jpeg_amd_timer_end(jpeg_amd_ctx *ctx, float *elapsed_ms);

/* ---- decode stages (device-resident) ---------------------------------------------- */

/* Spectral.Plane.idct(quanta:precision:)  decode.swift:4101-4133 (+ modulate :3984-4017,
 * load :4020-4039, idct8 :4042-4093, idct8x8 :4095-4099).  One plane. */
int jpeg_amd_idct_plane(jpeg_amd_ctx *ctx, const int16_t *d_coef, int units_x, int units_y,
                        const uint16_t h_quanta_zigzag[64], int precision,
                        uint16_t *d_plane);

/* Spectral.idct()  decode.swift:4154-4165: every plane of an image.
 * h_quanta: [ntables][64] zigzag; plane p uses table layout->qi[p]. */
int jpeg_amd_spectral_idct(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout,
                           const int16_t *const d_coef[], const uint16_t *h_quanta,
                           int ntables, uint16_t *const d_planes[]);

/* Planar.interleaved(cosite:)  decode.swift:4182-4276 */
int jpeg_amd_planar_interleaved(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout,
                                const uint16_t *const d_planes[], int cosited,
                                uint16_t *d_rect);

/* Rectangular.unpack(as:) for the built-in 8-bit colour targets  decode.swift:4291-4298.
 * nplanes = 1 (y8 / nonconforming1x8) or 3 (ycc8 / nonconforming3x8). */
int jpeg_amd_rectangular_unpack(jpeg_amd_ctx *ctx, const uint16_t *d_rect, size_t npixels,
                                int nplanes, jpeg_amd_color color, uint8_t *d_pixels);

/* Fused Spectral -> pixels: == idct().interleaved(cosite:).unpack(as:) bit for bit,
 * without materialising Planar / Rectangular in HBM (8-bit formats, 1 or 3 planes).
 * n_images images of identical layout; image i reads d_coef[p] + i*coef_stride[p]
 * (int16 elements), table set i*quanta_stride (uint16 elements) of d_quanta and writes
 * d_pixels + i*pixel_stride (bytes).  d_quanta: DEVICE pointer [..][ntables][64]. */
int jpeg_amd_decode_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, int n_images,
                          const int16_t *const d_coef[], const size_t coef_stride[],
                          const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                          int cosited, jpeg_amd_color color,
                          uint8_t *d_pixels, size_t pixel_stride);
/* single image, host tables */
int jpeg_amd_decode(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout,
                    const int16_t *const d_coef[], const uint16_t *h_quanta, int ntables,
                    int cosited, jpeg_amd_color color, uint8_t *d_pixels);

/* Fused Spectral -> Rectangular: == idct().interleaved(cosite:) bit for bit (decode.swift:4154-4165, 4182-4276) -- what
 * Rectangular.decompress(stream:cosite:) runs behind the entropy decoder (decode.swift:4367-4374) -- for ANY JPEG.Format
 * (jpeg.swift:21-56; examples/custom-color/main.swift:41-63): precision 1 .. 16, 1 .. 4 planes, centred or cosited.
 * Layouts whose planes lie at the image's scale or at half of it per axis (factors 1 | 2, scale <= 2) take ONE launch with no
 * Planar intermediate in HBM (kernels_generic.hip; the reference's literal operation sequence: true division, .rounded());
 * every other layout (factors 3, 4 ...) runs the staged kernels through the context's scratch -- same result either way.
 * d_rect: uint16 [H][W][nplanes]; batch strides as in jpeg_amd_decode_batch (rect_stride in uint16 elements). */
int jpeg_amd_spectral_rectangular_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, int n_images,
                                        const int16_t *const d_coef[], const size_t coef_stride[],
                                        const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                        int cosited, uint16_t *d_rect, size_t rect_stride);
/* single image, host tables */
int jpeg_amd_spectral_rectangular(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout,
                                  const int16_t *const d_coef[], const uint16_t *h_quanta, int ntables,
                                  int cosited, uint16_t *d_rect);

/* Fused Rectangular -> Spectral: == decomposed().fdct(quanta:) bit for bit (encode.swift:389-425, 199-248) -- what
 * Rectangular.compress(stream:quanta:) runs in front of the entropy coder (encode.swift:2031) -- for ANY JPEG.Format, the
 * mirror image of jpeg_amd_spectral_rectangular: the layouts that take one launch there take one here (no Planar
 * intermediate in HBM, the reference's literal operation sequence), every other layout runs the staged kernels through the
 * context's scratch.  d_rect: uint16 [H][W][nplanes]; d_coef[p]: int16 [units_y][units_x][64], zigzag. */
int jpeg_amd_rectangular_spectral_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, int n_images,
                                        const uint16_t *d_rect, size_t rect_stride, const uint16_t *d_quanta,
                                        size_t quanta_stride, int ntables, int16_t *const d_coef[],
                                        const size_t coef_stride[]);
/* single image, host tables */
int jpeg_amd_rectangular_spectral(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, const uint16_t *d_rect,
                                  const uint16_t *h_quanta, int ntables, int16_t *const d_coef[]);

/* ---- encode stages (device-resident) ---------------------------------------------- */

/* Rectangular.pack(size:layout:metadata:pixels:)  encode.swift:453-464 */
int jpeg_amd_rectangular_pack(jpeg_amd_ctx *ctx, const uint8_t *d_pixels, size_t npixels,
                              int nplanes, jpeg_amd_color color, uint16_t *d_rect);

/* Rectangular.decomposed()  encode.swift:389-425 */
int jpeg_amd_rectangular_decomposed(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout,
                                    const uint16_t *d_rect, uint16_t *const d_planes[]);

/* Spectral.Plane.fdct(_:quanta:precision:)  encode.swift:199-248 */
int jpeg_amd_fdct_plane(jpeg_amd_ctx *ctx, const uint16_t *d_plane, int units_x, int units_y,
                        const uint16_t h_quanta_zigzag[64], int precision, int16_t *d_coef);

/* Planar.fdct(quanta:)  encode.swift:353-370 */
int jpeg_amd_planar_fdct(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout,
                         const uint16_t *const d_planes[], const uint16_t *h_quanta,
                         int ntables, int16_t *const d_coef[]);

/* Fused pixels -> Spectral: == pack(...).decomposed().fdct(quanta:) bit for bit
 * (8-bit formats, 1 or 3 planes).  Strides as in jpeg_amd_decode_batch. */
int jpeg_amd_encode_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, int n_images,
                          const uint8_t *d_pixels, size_t pixel_stride, jpeg_amd_color color,
                          const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                          int16_t *const d_coef[], const size_t coef_stride[]);
int jpeg_amd_encode(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout,
                    const uint8_t *d_pixels, jpeg_amd_color color,
                    const uint16_t *h_quanta, int ntables, int16_t *const d_coef[]);

/* ---- host-buffer conveniences: what the Swift shim calls ---------------------------
 * Same semantics as the calls above with every buffer in HOST memory: the library
 * uploads inputs, runs the kernels and downloads outputs (synchronous). */
int jpeg_amd_host_spectral_idct(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout,
                                const int16_t *const h_coef[], const uint16_t *h_quanta,
                                int ntables, uint16_t *const h_planes[]);
int jpeg_amd_host_planar_interleaved(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout,
                                     const uint16_t *const h_planes[], int cosited,
                                     uint16_t *h_rect);
int jpeg_amd_host_rectangular_unpack(jpeg_amd_ctx *ctx, const uint16_t *h_rect,
                                     size_t npixels, int nplanes, jpeg_amd_color color,
                                     uint8_t *h_pixels);
int jpeg_amd_host_decode(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout,
                         const int16_t *const h_coef[], const uint16_t *h_quanta, int ntables,
                         int cosited, jpeg_amd_color color, uint8_t *h_pixels);
/* idct().interleaved(cosite:) with host buffers: ONE crossing of the link each way, one launch on the device for formats
 * whose planes lie at the image's scale or at half of it (jpeg_amd_spectral_rectangular). */
int jpeg_amd_host_spectral_rectangular(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout,
                                       const int16_t *const h_coef[], const uint16_t *h_quanta, int ntables,
                                       int cosited, uint16_t *h_rect);
/* decomposed().fdct(quanta:) with host buffers, likewise (jpeg_amd_rectangular_spectral) */
int jpeg_amd_host_rectangular_spectral(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, const uint16_t *h_rect,
                                       const uint16_t *h_quanta, int ntables, int16_t *const h_coef[]);
int jpeg_amd_host_rectangular_pack(jpeg_amd_ctx *ctx, const uint8_t *h_pixels, size_t npixels,
                                   int nplanes, jpeg_amd_color color, uint16_t *h_rect);
int jpeg_amd_host_rectangular_decomposed(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout,
                                         const uint16_t *h_rect, uint16_t *const h_planes[]);
int jpeg_amd_host_planar_fdct(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout,
                              const uint16_t *const h_planes[], const uint16_t *h_quanta,
                              int ntables, int16_t *const h_coef[]);
int jpeg_amd_host_encode(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout,
                         const uint8_t *h_pixels, jpeg_amd_color color,
                         const uint16_t *h_quanta, int ntables, int16_t *const h_coef[]);

/* ---- host side of the path's INPUT ("next" rows) -------------------------
 * Huffman entropy decoding stays on the host CPU (north_star); these entry points turn a JPEG
 * byte stream into the Spectral containers the kernels consume, like
 * JPEG.Data.Spectral.decompress(stream:) does through JPEG.Context (decode.swift:3554-3961,
 * 4315).  Baseline / extended sequential and progressive Huffman, restart intervals, 1..4
 * components, 8-bit or 12-bit.  No GPU is needed for the first two. */
typedef struct jpeg_amd_frame_info {
    int32_t width, height, precision, ncomponents;
    int32_t process;                          /* 0 baseline, 1 extended sequential, 2 progressive */
    int32_t scale_x, scale_y;                 /* Layout.scale */
    int32_t id[JPEG_AMD_MAX_PLANES];          /* component identifiers, frame order */
    int32_t factor_x[JPEG_AMD_MAX_PLANES], factor_y[JPEG_AMD_MAX_PLANES];
    int32_t units_x[JPEG_AMD_MAX_PLANES], units_y[JPEG_AMD_MAX_PLANES];
    int32_t nscans, restart_interval;
} jpeg_amd_frame_info;

/* JPEG.Table.Huffman<Symbol>.Decoder subscript  decode.swift:1243-1261 (table construction :1008-1240): build the
 * decoder of a DHT table -- counts[l] codewords of length l + 1, `values` in codeword order -- and decode the
 * codeword at the top of the 16-bit window `window` (big-endian, left-aligned).  A window that is no codeword gives
 * symbol 0 and length 16: the reference renders damaged streams that way instead of failing, and so does
 * jpeg_amd_jpeg_decode_spectral.  EINVAL for tables the reference's initialiser rejects (over-subscribed lengths,
 * more than 256 values).  Known-answer vectors: tests/unit/tests.swift:141-461.  Host only. */
int jpeg_amd_huffman_lookup(const uint8_t counts[16], const uint8_t *values, int nvalues,
                            uint16_t window, int32_t *symbol, int32_t *length);
/* JPEG.Table.Huffman<Symbol>.init(frequencies:target:)  encode.swift:597-760: the code Spectral.compress builds for
 * a scan from its symbol frequencies (optimal lengths, the reference's tie-breaking and its 16-bit limiter), as a
 * DHT table: counts[16], values[] in codeword order (*nvalues of them, <= 256).  freq[v] <= 0: symbol unused. */
int jpeg_amd_huffman_build(const int64_t freq[256], uint8_t counts[16], uint8_t values[256], int32_t *nvalues);

/* parse the headers (and walk the scans) without decoding: geometry for buffer allocation */
int jpeg_amd_jpeg_inspect(const uint8_t *h_jpeg, size_t nbytes, jpeg_amd_frame_info *info);
/* entropy-decode every scan into caller-allocated planes h_coef[c]: int16 [units_y][units_x][64]
 * zigzag (zeroed here first); h_quanta[c] receives the table bound to component c (zigzag).
 * Damaged entropy-coded data is decoded the way the reference decodes it, not refused: a 16-bit window that matches
 * no codeword is symbol 0 of length 16 (decode.swift:1255-1258), a stream that ends early is padded with 1-bits. */
int jpeg_amd_jpeg_decode_spectral(const uint8_t *h_jpeg, size_t nbytes, int16_t *const h_coef[],
                                  uint16_t h_quanta[][64], jpeg_amd_frame_info *info);
/* The same with the restart intervals of every scan decoded by `nthreads` host threads
 * (<= 0: all cores): intervals are independent bit streams (DC predictors and EOB runs reset at
 * RSTn, decode.swift:3210, 3500-3502).  Files without DRI, or with a damaged marker sequence,
 * take the sequential path. */
int jpeg_amd_jpeg_decode_spectral_mt(const uint8_t *h_jpeg, size_t nbytes, int16_t *const h_coef[],
                                     uint16_t h_quanta[][64], jpeg_amd_frame_info *info, int nthreads);
/* The image as it stands after the first `max_scans` scans (0 = all): what JPEG.Context hands out
 * between scans (decode.swift:3554-3961, examples/decode-online) -- progressive previews.
 * Components no scan has reached yet are all zero and get a table of ones. */
int jpeg_amd_jpeg_decode_spectral_partial(const uint8_t *h_jpeg, size_t nbytes, int16_t *const h_coef[],
                                          uint16_t h_quanta[][64], jpeg_amd_frame_info *info,
                                          int nthreads, int max_scans);
/* A decoder fed by a GROWING byte stream -- JPEG.Context driven by a Bytestream.Source that runs
 * dry (decode.swift:3554-3961; examples/decode-online): push whatever bytes have arrived; every
 * segment and every scan that is complete by then is consumed, incomplete ones wait for the next
 * push.  *scans_done counts the scans decoded so far, *finished is set at EOI.  The decoder owns
 * the planes; jpeg_amd_stream_snapshot copies them (and the table of every component, ones for a
 * component no scan has reached yet) into caller buffers sized from jpeg_amd_stream_info.
 * Because it owns the planes it refuses frames of more than 32 Mi blocks in all (ENOMEM; larger frames go through
 * the one-shot entry points, where the caller allocates), and its first error is final: every later push returns
 * the same status without touching the decoder's state. */
/* The same file as SPARSE coefficients: one 32-bit entry per nonzero coefficient (every block's DC has one) --
 * bits 0-15 the int16 coefficient, bits 16-21 its zigzag index, bit 31 set on the last entry of its block -- the entries of a
 * block in a row, and per block of the frame (planes in frame order, plane c's block (x, y) at
 * sum(units_x * units_y of the planes before c) + y * units_x + x) the index of its first entry in h_desc, 0xFFFFFFFF for a
 * block no scan reached.  What the host has to write and PCIe has to carry is an eighth of the planes for a typical file;
 * jpeg_amd_spectral_expand rebuilds the planes on the device.  Sequential files with every restart marker in place only:
 * JPEG_AMD_ENOSUP for anything else (progressive, a damaged marker sequence) and when `capacity` entries do not suffice --
 * decode those with jpeg_amd_jpeg_decode_spectral. */
int jpeg_amd_jpeg_decode_sparse(const uint8_t *data, size_t nbytes, uint32_t *h_desc, size_t ndesc,
                                uint32_t *h_entries, size_t capacity, size_t *nentries,
                                uint16_t h_quanta[][64], jpeg_amd_frame_info *info);

/* ---- entropy decoding on the device: one restart interval per work-item ------------------------------------------------
 * The restart intervals of a sequential scan are independent bit streams (T.81 E.2.4): k_huffman_intervals decodes one per
 * work-item, from the file's entropy-coded bytes in device memory into Spectral planes in device memory.  The decoder is
 * csrc/huffman_interval.hpp, one statement for the kernel and for the host.
 *
 * jpeg_amd_jpeg_plan_intervals: whether a file takes that route, judged on the host from its headers and marker positions
 * alone, and how much work it is (*nscans scans, *nintervals intervals in all; a file without DRI is one interval per scan).
 *   JPEG_AMD_OK      a sequential Huffman frame, every scan of it sequential (interleaved or not), with every restart marker
 *                    where DRI says it is -- the files jpeg_amd_jpeg_decode_sparse takes, however dense
 *   JPEG_AMD_ENOSUP  a progressive frame; a missing or surplus restart marker; more than 16 blocks in an MCU; more than
 *                    JPEG_AMD_MAX_DEVICE_INTERVALS intervals in the file; a component that two scans write (the device
 *                    decodes all scans at once, and the later scan has to win)
 *   JPEG_AMD_EINVAL  what jpeg_amd_jpeg_inspect and the entropy decoder call malformed, a scan that names an undefined
 *                    Huffman table or an unbound quantisation table included
 * Host only. */
#define JPEG_AMD_MAX_DEVICE_INTERVALS (1 << 20)
int jpeg_amd_jpeg_plan_intervals(const uint8_t *h_jpeg, size_t nbytes, jpeg_amd_frame_info *info, int32_t *nscans,
                                 int64_t *nintervals);
/* The host instantiation of the same decoder over the same work list, one interval after the other, into host planes: what
 * the kernel computes, without a device.  Planes, tables and status are jpeg_amd_jpeg_decode_spectral's for every file the
 * planner takes (the planner's status otherwise, with nothing written); the planes need no alignment. */
int jpeg_amd_jpeg_decode_intervals_host(const uint8_t *h_jpeg, size_t nbytes, int16_t *const h_coef[],
                                        uint16_t h_quanta[][64], jpeg_amd_frame_info *info);
/* n_images files of ANY mix of geometries, entropy-decoded on the device.  File i writes whole planes d_coef[i][c] (device
 * memory, int16 [units_y][units_x][64] zigzag, sized from jpeg_amd_jpeg_inspect, 16-byte aligned): byte for byte the planes
 * of jpeg_amd_jpeg_decode_spectral, every block of every plane written.  h_quanta[i][c] and h_info[i] receive what that call
 * gives; h_status[i] the file's status, the first that is not OK among its intervals in file order.
 * Judged before anything is enqueued, the context last: a null pointer (EINVAL; of d_coef[i] the first ncomponents entries
 * count) or a misaligned plane (EINVAL), a file the planner refuses (its status, for the whole call, nothing written).
 * n_images == 0 is OK.  One upload (the entropy-coded bytes, the tables and the work list), one launch; the call waits and
 * returns the first h_status[i] that is not OK.  The planes of a file whose status is not OK are unspecified. */
int jpeg_amd_jpeg_decode_spectral_device(jpeg_amd_ctx *ctx, int n_images, const uint8_t *const h_jpeg[], const size_t nbytes[],
                                         int16_t *const d_coef[][JPEG_AMD_MAX_PLANES],
                                         uint16_t h_quanta[][JPEG_AMD_MAX_PLANES][64], jpeg_amd_frame_info *h_info,
                                         int32_t *h_status);
/* How many files the context has entropy-decoded on the device since it was made: those of
 * jpeg_amd_jpeg_decode_spectral_device, and those that took the device route of the batch file calls. */
int jpeg_amd_ctx_device_entropy_files(const jpeg_amd_ctx *ctx, int64_t *count);
/* ... and the time k_huffman_intervals itself has taken for them, in milliseconds (HIP events around every launch). */
int jpeg_amd_ctx_device_entropy_kernel_ms(const jpeg_amd_ctx *ctx, double *ms);

/* Sparse coefficients -> Spectral planes on the device (the other half of jpeg_amd_jpeg_decode_sparse): image i reads its
 * descriptors at d_desc + i * desc_stride and its entries at d_entries + i * entries_stride (elements) and has every block
 * of its planes d_coef[p] + i * coef_stride[p] written; d_skip (optional, one byte per image): nonzero = the image's planes
 * are left as they are.  Asynchronous on the context's stream.  JPEG_AMD_EINVAL for a frame of 2^32 - 1 blocks or more
 * (descriptors are 32-bit indices, and 0xFFFFFFFF means no block). */
int jpeg_amd_spectral_expand_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, int n_images,
                                   const uint32_t *d_desc, size_t desc_stride, const uint32_t *d_entries,
                                   size_t entries_stride, const uint8_t *d_skip, int16_t *const d_coef[],
                                   const size_t coef_stride[]);

/* Spectral planes -> sparse coefficients on the device, the way back (what the batch compress calls run in front of
 * jpeg_amd_jpeg_encode_sparse): image i reads its planes at d_coef[p] + i * coef_stride[p] and writes its descriptors at
 * d_desc + i * desc_stride and its entries into the arena of `capacity` entries at d_entries + i * entries_stride (elements).
 * Per block, planes in frame order: an entry for index 0 always, then one for every nonzero coefficient in ascending zigzag
 * order, the last one flagged; the rows of the blocks lie in the arena in no particular order -- the descriptors say where.
 *   d_count[i] is image i's entry count, whether the entries fit or not.
 *   d_count[i] <= capacity: every descriptor of image i is written, and the rows tile [0, d_count[i]) of its arena, without
 *     holes and without overlap; nothing behind them is written.
 *   d_count[i] > capacity: the descriptors and entries of image i are unspecified, but nothing outside [0, capacity) of its
 *     arena is written.
 * Asynchronous on the context's stream.  JPEG_AMD_EINVAL for a frame of 2^26 blocks or more: the count is kept in 32 bits
 * and takes up to 64 per block. */
int jpeg_amd_spectral_sparsify_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, int n_images,
                                     const int16_t *const d_coef[], const size_t coef_stride[], uint32_t *d_desc,
                                     size_t desc_stride, uint32_t *d_entries, size_t entries_stride, uint32_t capacity,
                                     uint32_t *d_count);

typedef struct jpeg_amd_stream jpeg_amd_stream;
jpeg_amd_stream *jpeg_amd_stream_create(void);
void jpeg_amd_stream_destroy(jpeg_amd_stream *stream);
int jpeg_amd_stream_push(jpeg_amd_stream *stream, const uint8_t *h_bytes, size_t nbytes, int *scans_done,
                         int *finished);
int jpeg_amd_stream_info(const jpeg_amd_stream *stream, jpeg_amd_frame_info *info);
int jpeg_amd_stream_snapshot(const jpeg_amd_stream *stream, int16_t *const h_coef[], uint16_t h_quanta[][64]);
/* Rectangular.decompress(stream:cosite:) + unpack(as:)  (decode.swift:4367, os.swift:375):
 * JPEG bytes in, H*W colours of 3 bytes out (host memory); 8-bit images of 1 or 3 components. */
int jpeg_amd_decompress(jpeg_amd_ctx *ctx, const uint8_t *h_jpeg, size_t nbytes, int cosited,
                        jpeg_amd_color color, uint8_t *h_pixels, size_t pixel_capacity,
                        jpeg_amd_frame_info *info);

/* Rectangular<Format>.decompress(stream:cosite:) for ANY JPEG.Format  (decode.swift:4367-4374; what
 * examples/custom-color/main.swift:190-200 does with its 12-bit four-component format): JPEG bytes in host memory ->
 * entropy decoding on the host (restart intervals on `nthreads` threads, <= 0: all cores) -> idct() + interleaved(cosite:)
 * on the GPU -> the samples, uint16 [H][W][n], in host memory.  n = nrecognized, the first nrecognized components of the
 * frame (0: all of them); the components behind them are non-recognised by the format (jpeg.swift:21-56): they take part in
 * the image's scale and in nothing else.  Precision 1 .. 16, 1 .. 4 components, sequential or progressive, any sampling
 * factors.  rect_capacity: the size of h_rect in samples (H * W * n are written; EINVAL if it is smaller). */
int jpeg_amd_decompress_rectangular(jpeg_amd_ctx *ctx, const uint8_t *h_jpeg, size_t nbytes, int cosited,
                                    int nrecognized, int nthreads, uint16_t *h_rect, size_t rect_capacity,
                                    jpeg_amd_frame_info *info);

/* The same for n_images files of ONE frame geometry (a burst, the frames of an MJPEG stream):
 * `nthreads` host threads (<= 0: all cores) entropy-decode into pinned buffers, the device decodes
 * a chunk of images per launch.  h_pixels: image i at h_pixels + i * pixel_stride (0 = W*H*3).
 * This is the restart-interval / image-level parallelism of SURVEY.md 8f-1 on the host side.
 * h_pixels may be pageable (downloaded into the context's pinned slots, copied out by the host threads) or page-locked
 * (hipHostMalloc / hipHostRegister: downloaded straight into it).
 * Threads: the calling thread directs (it submits chunks to the device and polls their events); `nthreads` threads beside it
 * entropy-decode, and for pageable output up to min(nthreads, 16) more copy pixels out of the pinned slots -- all of them kept
 * in the context between calls.  If no helper thread can be started the call runs synchronously on the calling thread. */
int jpeg_amd_decompress_batch(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                              int n_images, int nthreads, int cosited, jpeg_amd_color color,
                              uint8_t *h_pixels, size_t pixel_stride, jpeg_amd_frame_info *info);
/* The same, with the pixels LEFT ON THE DEVICE (image i at d_pixels + i * pixel_stride): what crosses PCIe is the sparse form
 * of the coefficients (jpeg_amd_jpeg_decode_sparse) -- about 0.8 MB instead of 6.2 MB for a typical 1080p file -- and nothing
 * comes back.  Returns when the last chunk's kernels have finished. */
int jpeg_amd_decompress_batch_device(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                                     int n_images, int nthreads, int cosited, jpeg_amd_color color,
                                     uint8_t *d_pixels, size_t pixel_stride, jpeg_amd_frame_info *info);

/* ---- host side of the path's OUTPUT ("next" row) ------------------------------
 * The Huffman entropy encoder and file writer behind JPEG.Data.Spectral.compress(stream:)
 * (encode.swift:1918-1972): optimised Huffman tables per scan (:700-760), sequential scans,
 * interleaved or not (:962-1011, 1211-1384), table definitions grouped like
 * JPEG.Layout.definitions (jpeg.swift:1383-1442).  Output is byte-identical to the reference's
 * files for the same coefficients.  Sequential and progressive (DC / AC, first pass and
 * refinement, EOB runs: encode.swift:1013-1206, 1386-1557) Huffman scans. */
typedef struct jpeg_amd_scan {                /* JPEG.Header.Scan (jpeg.swift:1640-1760) */
    int32_t ncomponents;
    int32_t component[JPEG_AMD_MAX_PLANES];   /* plane indices (frame order), ascending */
    int32_t dc[JPEG_AMD_MAX_PLANES];          /* Huffman table selectors 0..1 (baseline) / 0..3 */
    int32_t ac[JPEG_AMD_MAX_PLANES];
    /* progressive process only; all zero = a sequential scan (.sequential(...)):
     *   band_lo = 0, band_hi = 1, refine = 0: .progressive(..., bits: bit...)     DC, first pass
     *   band_lo = 0, band_hi = 1, refine = 1: .progressive(..., bit: bit)         DC, one more bit
     *   band_lo >= 1,             refine = 0: .progressive(c, band:, bits: bit...) AC, first pass
     *   band_lo >= 1,             refine = 1: .progressive(c, band:, bit: bit)     AC, one more bit */
    int32_t band_lo, band_hi;                 /* zigzag band [band_lo, band_hi) */
    int32_t bit, refine;
} jpeg_amd_scan;

typedef struct jpeg_amd_jfif {                /* JPEG.JFIF */
    int32_t version_minor;                    /* 1.0, 1.1, 1.2 -> 0, 1, 2 */
    int32_t unit;                             /* 0 none, 1 dots per inch, 2 dots per centimetre */
    int32_t density_x, density_y;
} jpeg_amd_jfif;

typedef struct jpeg_amd_metadata {            /* JPEG.Metadata record, written after SOI in order */
    int32_t kind;                             /* 0 .jfif, 1 .application(app, data:), 2 .comment(data:) */
    int32_t app;                              /* kind 1: 0..15 */
    jpeg_amd_jfif jfif;                       /* kind 0 */
    const uint8_t *data;                      /* kinds 1, 2: segment payload */
    size_t size;
} jpeg_amd_metadata;

/* frame: width, height, precision, process (0 baseline, 1 extended), ncomponents, id[] (ascending),
 * factor_*[], units_*[] of the planes in h_coef[] (int16 [units_y][units_x][64], zigzag).
 * quanta_key[c]: quantisation-table key of component c (JPEG.Table.Quantization.Key);
 * h_quanta / h_quanta_keys: ntables tables of 64 zigzag values and their keys.
 * process 2 (progressive) takes progressive scans, 0 / 1 sequential ones.
 * frame->restart_interval > 0 (an extension: the reference's writer never emits DRI) cuts every
 * scan into restart intervals of that many MCUs, which the decoder then takes on several threads.
 * h_out == NULL only computes *nbytes. */
int jpeg_amd_jpeg_encode_spectral(const jpeg_amd_frame_info *frame, const int32_t *quanta_key,
                                  const int16_t *const h_coef[], const uint16_t *h_quanta,
                                  const int32_t *h_quanta_keys, int ntables,
                                  const jpeg_amd_scan *scans, int nscans,
                                  const jpeg_amd_metadata *metadata, int nmetadata, uint8_t *h_out,
                                  size_t capacity,
                                  size_t *nbytes);
/* The same writer fed with SPARSE coefficients (the format of jpeg_amd_jpeg_decode_sparse: h_desc one descriptor per block of the
 * frame, planes in frame order; h_entries / nentries the arena; a block's entries in ascending zigzag index, the DC first):
 * sequential scans only (JPEG_AMD_ENOSUP for a progressive frame).  Byte-identical to jpeg_amd_jpeg_encode_spectral on the
 * planes those entries expand to.  jpeg_amd_compress_batch brings the coefficients down from the device in this form. */
int jpeg_amd_jpeg_encode_sparse(const jpeg_amd_frame_info *frame, const int32_t *quanta_key, const uint32_t *h_desc,
                                const uint32_t *h_entries, size_t nentries, const uint16_t *h_quanta,
                                const int32_t *h_quanta_keys, int ntables, const jpeg_amd_scan *scans, int nscans,
                                const jpeg_amd_metadata *metadata, int nmetadata, uint8_t *h_out, size_t capacity,
                                size_t *nbytes);
/* Rectangular.pack(...).compress(stream:quanta:)  (encode.swift:456, 2031; os.swift:412): H*W
 * colours of 3 bytes in host memory -> colour conversion, downsampling, FDCT and quantisation on
 * the GPU -> entropy coding on the host -> JPEG bytes.  8-bit, 1 or 3 components, ids in
 * frame->id.  frame->units_* are filled in. */
int jpeg_amd_compress(jpeg_amd_ctx *ctx, jpeg_amd_frame_info *frame, const uint8_t *h_pixels,
                      jpeg_amd_color color, const int32_t *quanta_key, const uint16_t *h_quanta,
                      const int32_t *h_quanta_keys, int ntables, const jpeg_amd_scan *scans,
                      int nscans, const jpeg_amd_metadata *metadata, int nmetadata, uint8_t *h_out,
                      size_t capacity,
                      size_t *nbytes);

/* Rectangular<Format>.compress(stream:quanta:) for ANY JPEG.Format  (encode.swift:2031; examples/custom-color/
 * main.swift:132-188): samples uint16 [H][W][frame->ncomponents] in host memory -> decomposed() + fdct(quanta:) on the GPU
 * -> entropy coding on the host -> JPEG bytes.  frame: width, height, precision (1 .. 16), process, ncomponents (1 .. 4),
 * id[] (ascending), factor_*[]; units_* and scale_* are filled in.  Tables, scans and metadata as for jpeg_amd_compress
 * (quanta above 255 are written as 16-bit tables).  h_out == NULL only computes *nbytes. */
int jpeg_amd_compress_rectangular(jpeg_amd_ctx *ctx, jpeg_amd_frame_info *frame, const uint16_t *h_rect,
                                  const int32_t *quanta_key, const uint16_t *h_quanta,
                                  const int32_t *h_quanta_keys, int ntables, const jpeg_amd_scan *scans,
                                  int nscans, const jpeg_amd_metadata *metadata, int nmetadata, uint8_t *h_out,
                                  size_t capacity, size_t *nbytes);

/* The same for n_images pictures of ONE geometry, tables and scan progression: image i at
 * h_pixels + i * pixel_stride (0 = W*H*3); file i is written to h_out + i * out_stride and is
 * nbytes[i] long (EINVAL with nbytes[i] > out_stride: that buffer was too small).  One fused
 * encode launch per chunk, the entropy coding on `nthreads` host threads (<= 0: all cores). */
int jpeg_amd_compress_batch(jpeg_amd_ctx *ctx, jpeg_amd_frame_info *frame, const uint8_t *h_pixels,
                            size_t pixel_stride, int n_images, jpeg_amd_color color,
                            const int32_t *quanta_key, const uint16_t *h_quanta,
                            const int32_t *h_quanta_keys, int ntables, const jpeg_amd_scan *scans,
                            int nscans, const jpeg_amd_metadata *metadata, int nmetadata, int nthreads,
                            uint8_t *h_out, size_t out_stride, size_t nbytes[]);
/* The same with the pixels ALREADY ON THE DEVICE (picture i at d_pixels + i * pixel_stride): nothing is uploaded, the
 * coefficients come down and the files are written into host memory as above. */
int jpeg_amd_compress_batch_device(jpeg_amd_ctx *ctx, jpeg_amd_frame_info *frame, const uint8_t *d_pixels,
                            size_t pixel_stride, int n_images, jpeg_amd_color color,
                            const int32_t *quanta_key, const uint16_t *h_quanta,
                            const int32_t *h_quanta_keys, int ntables, const jpeg_amd_scan *scans,
                            int nscans, const jpeg_amd_metadata *metadata, int nmetadata, int nthreads,
                            uint8_t *h_out, size_t out_stride, size_t nbytes[]);

/* ---- lossless spectral transforms: rotate, flip, crop, requantise --------------------------------
 * Editing JPEG.Data.Spectral directly, as examples/rotate/main.swift (lossless 90 / 180 / 270 degree rotations) and
 * examples/recompress/main.swift:40-61 (new quantisation tables without going back to pixels) do.
 *
 * op: three bits applied in this order -- TRANSPOSE (across the main diagonal), then FLIP_H (mirror left-right), then
 * FLIP_V (mirror top-bottom).  The 8 results are the dihedral group; the reference's rotations are
 *   "ii"  = ROT_CCW = reflectVertical(transpose)    (90 degrees counter-clockwise, np.rot90(k=1))
 *   "iii" = ROT_180 = reflectVertical(reflectHorizontal)
 *   "iv"  = ROT_CW  = reflectHorizontal(transpose).
 * Inside a block (the example's Block.transform): output zigzag index z takes sign(z) * in[m(z)]; a transpose swaps the
 * frequencies (k, h), a horizontal mirror negates odd k, a vertical mirror negates odd h.  Tables: q_out[z] = q_in[m(z)].
 * Block grid (the example's matrix / offset): block (x, y) of a plane goes to its transposed and / or mirrored position
 * among that plane's units.
 * Region (optional, source pixels, applied BEFORE the op): x, y multiples of 8 * scale_x, 8 * scale_y and inside the image,
 * width, height > 0; it may reach past the image, and the blocks it adds are zero -- with x = y = 0 it is exactly
 * Spectral.set(width:) / set(height:) (decode.swift:2443-2500).
 * Trim (the example's rule): after the region, a partial-MCU edge the op would move to the top or left is cut to whole MCUs
 * -- a mirrored source x (FLIP_H without TRANSPOSE, FLIP_V with it: ROT_CCW, ROT_180) trims the width, a mirrored source y
 * (FLIP_V without TRANSPOSE, FLIP_H with it: ROT_CW, ROT_180) the height.  Partial edges that stay right / bottom are kept.
 * Layout: a transposing op swaps factor_x / factor_y of every plane and scale_x / scale_y (4:2:2 becomes 4:4:0); units are
 * recomputed as in jpeg_amd_layout_units.
 * Requantisation (optional; new tables in OUTPUT orientation), examples/recompress/main.swift:52-56:
 *   v = Int16(q_in[m(z)]) * sign(z) * in[m(z)];  r = Double(v) / Double(q_out[z]);  out = Int16(r + 0.3 * (r < 0 ? -1 : 1))
 * (truncation toward zero).  Where the reference traps the call fails with EINVAL: q_in > 32767, an Int16 product that
 * overflows (a negated -32768 included, which also holds without requantisation), q_out = 0.  Without requantisation the
 * coefficients are copied exactly. */
#define JPEG_AMD_XFORM_TRANSPOSE 1
#define JPEG_AMD_XFORM_FLIP_H    2
#define JPEG_AMD_XFORM_FLIP_V    4
#define JPEG_AMD_XFORM_NONE       0
#define JPEG_AMD_XFORM_ROT_CCW    (JPEG_AMD_XFORM_TRANSPOSE | JPEG_AMD_XFORM_FLIP_V)   /* "ii"  */
#define JPEG_AMD_XFORM_ROT_180    (JPEG_AMD_XFORM_FLIP_H | JPEG_AMD_XFORM_FLIP_V)      /* "iii" */
#define JPEG_AMD_XFORM_ROT_CW     (JPEG_AMD_XFORM_TRANSPOSE | JPEG_AMD_XFORM_FLIP_H)   /* "iv"  */
#define JPEG_AMD_XFORM_TRANSVERSE 7

typedef struct jpeg_amd_region {
    int32_t x, y, width, height;              /* source pixels */
} jpeg_amd_region;

/* The output geometry of `op` and `region` (NULL = the whole image) applied to `in`; qi is carried over.  EINVAL for an
 * unaligned or outside origin, a zero size, or a trim that leaves nothing.  Host only. */
int jpeg_amd_transform_layout(const jpeg_amd_layout *in, int op, const jpeg_amd_region *region, jpeg_amd_layout *out);
/* q_out[z] = q_in[m(z)].  Host only. */
int jpeg_amd_transform_quanta(int op, const uint16_t in[64], uint16_t out[64]);
/* One launch for every plane of n_images images of layout in_layout: image i of plane p reads d_coef_in[p] +
 * i * in_stride[p] and writes d_coef_out[p] + i * out_stride[p] (int16 elements; the output planes are sized by
 * jpeg_amd_transform_layout).  d_quanta: DEVICE tables [..][ntables][64], image i at i * quanta_stride; plane p uses
 * table in_layout->qi[p].  d_quanta_out: NULL = no requantisation, else the new tables, output orientation, same layout
 * and strides.  d_overflow (optional): a device int32 the kernel sets to 1 where the reference would trap (it is not
 * cleared here).  Asynchronous on the ctx stream. */
int jpeg_amd_spectral_transform_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *in_layout, int n_images, int op,
                                      const jpeg_amd_region *region, const int16_t *const d_coef_in[],
                                      const size_t in_stride[], const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                      const uint16_t *d_quanta_out, int16_t *const d_coef_out[], const size_t out_stride[],
                                      int32_t *d_overflow);
/* single image, host tables (h_quanta_out NULL = no requantisation); synchronises, EINVAL where the reference would trap */
int jpeg_amd_spectral_transform(jpeg_amd_ctx *ctx, const jpeg_amd_layout *in_layout, int op, const jpeg_amd_region *region,
                                const int16_t *const d_coef_in[], const uint16_t *h_quanta, int ntables,
                                const uint16_t *h_quanta_out, int16_t *const d_coef_out[]);

/* The script of a JPEG file, as its writer laid it out: the scans in order (*nscans of them; scans == NULL only counts,
 * otherwise scan_capacity must hold them all), each component's quantisation-table key (the index, in file order, of the
 * DQT table definition its frame selector points at when its first scan starts -- the inverse of JPEG.Layout's slot
 * allocation, jpeg.swift:1383-1442) and the APPn / COM segments in front of the frame header (*nmetadata of them, kind 1 /
 * 2, `data` pointing INTO h_jpeg; NULL / capacity as for scans).  What jpeg_amd_jpeg_encode_spectral takes to write the
 * file again.  Host only. */
int jpeg_amd_jpeg_script(const uint8_t *h_jpeg, size_t nbytes, jpeg_amd_scan *scans, int scan_capacity, int *nscans,
                         int32_t quanta_key[JPEG_AMD_MAX_PLANES], jpeg_amd_metadata *metadata, int metadata_capacity,
                         int *nmetadata);
/* File to file: entropy decoding on the host (restart intervals on `nthreads` threads, <= 0: all cores), the transform on
 * the GPU, and the host writer keeping the input's process, component ids, scan script, table keys, restart interval and
 * metadata segments verbatim and in order.  Every component of the frame is transformed.  h_requant: NULL or
 * [ncomponents][64] in output orientation (components that share a key must get equal tables).  h_out == NULL only sizes
 * the output (*nbytes_out); out_info (optional) receives the output frame.  (Verbatim includes an Exif segment's Orientation
 * tag, which jpeg_amd_jpeg_orientation reads: a file rotated here still NAMES its old orientation; the tag is not reset.) */
int jpeg_amd_transform(jpeg_amd_ctx *ctx, const uint8_t *h_jpeg, size_t nbytes, int op, const jpeg_amd_region *region,
                       const uint16_t *h_requant, int nthreads, uint8_t *h_out, size_t capacity, size_t *nbytes_out,
                       jpeg_amd_frame_info *out_info);

/* ---- region decode: the pixels of a rectangle ----------------------------------------------------
 * == jpeg_amd_decode_batch(...) of the same arguments, then image i cropped to regions[i], bit for bit
 * (decode.swift:4154-4165, 4182-4276, 4291-4298).  Regions are in PIXELS, any alignment: x, y >= 0, width, height > 0,
 * x + width <= W, y + height <= H.  Output image i at d_pixels + i * pixel_stride: region.height rows of region.width * 3
 * bytes, no padding between rows; pixel_stride >= 3 * width_i * height_i for every i (any value, 0 included, when
 * n_images == 1).  h_regions is a HOST array of n_images regions; the call copies it before it returns, as it copies host
 * tables.  Every region is validated before anything is enqueued: on EINVAL nothing is written.  Argument rules as
 * jpeg_amd_decode_batch: 8-bit only (else ENOSUP), 1 or 3 planes, at most 65 535 images, n_images == 0 is OK.
 * Cost: for the layouts of the fused decode (y8; ycc8 with full-factor luma and chroma at 1x or 2x per axis, centred) one
 * launch that reads only the blocks of each region's window (jpeg_amd_region_window) and writes only region pixels.  Other
 * layouts (cosited, factors 3 or 4, ...) decode the whole images into context scratch and crop: correct, but as costly as a
 * full decode.  A call whose regions are all whole images is jpeg_amd_decode_batch. */
int jpeg_amd_decode_region_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, int n_images,
                                 const int16_t *const d_coef[], const size_t coef_stride[],
                                 const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                 int cosited, jpeg_amd_color color, const jpeg_amd_region *h_regions,
                                 uint8_t *d_pixels, size_t pixel_stride);
/* single image, host tables */
int jpeg_amd_decode_region(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, const int16_t *const d_coef[],
                           const uint16_t *h_quanta, int ntables, int cosited, jpeg_amd_color color,
                           const jpeg_amd_region *region, uint8_t *d_pixels);
/* Host only.  windows[p] (in BLOCKS of plane p, for p < nplanes; the rest are zeroed): the smallest block rectangle that
 * holds every sample of plane p the reference reads for some pixel of `region` -- for an upsampled plane both neighbours
 * i and min(i + 1, 8 * units - 1) of the interleave index formula (decode.swift:4182-4276; oracle/jpeg_oracle.c
 * orc_interleave_rows), zero-weight reads included; for a plane at full factor, or a single-plane image, the sample under
 * the pixel.  EINVAL for a region outside the image, or a layout whose planes do not cover it. */
int jpeg_amd_region_window(const jpeg_amd_layout *layout, int cosited, const jpeg_amd_region *region,
                           jpeg_amd_region windows[JPEG_AMD_MAX_PLANES]);

/* ---- scaled decode: 1/2, 1/4 and 1/8 size pixels straight from the coefficients -------------------
 * The reference has no scaled decode; this is its own transform with the odd half and the upper coefficients deleted,
 * followed by its own interleave and colour stage.  THE CONTRACT (the one statement of it):
 *
 * denom in {1, 2, 4, 8}, N = 8 / denom.  The image becomes (W', H') = (ceil(W N / 8), ceil(H N / 8)) pixels; plane p
 * becomes N units_x[p] x N units_y[p] samples, N x N per block.
 *
 * Table, for k, h < N:  q_N[h][k] = (rN[k] * rN[h]) * (0x1p-3 * Float(Q[z(k, h)])), left-associative like
 * Spectral.Plane.modulate (decode.swift:3984-4017), with rN[i] = r[8 i / N] of the reference's vector:
 * r4 = {1, 1.306562965, 1, 0.541196100}, r2 = {1, 1}, r1 = {1}.  The scale stays 0x1p-3 for every N: the N / 8 of the
 * size change and the 1 / N of the N-point transform cancel against the reference's 1 / 8.
 *
 * Butterfly over the inputs h[0 .. N-1] along the transformed axis; every statement is ONE binary32 operation, nothing
 * is contracted:
 *   N = 4 (idct8's even half, decode.swift:4042-4093, with h[0], h[1], h[2], h[3] in the places of its h0, h2, h4, h6):
 *     e = shift + h[0];  a0 = e + h[2];  a1 = e - h[2];  b = h[1] + h[3];  c = 1.414213562 * (h[1] - h[3]) - b;
 *     g = (a0 + b, a1 + c, a1 - c, a0 - b)
 *   N = 2:  e = shift + h[0];  g = (e + h[1], e - h[1])
 *   N = 1:  g = (shift + h[0])
 *
 * Passes, as Spectral.Plane.idct (decode.swift:4101-4133): the first over the vertical frequency of each column k < N
 * with no shift, the second over the horizontal frequency of each row with shift = level = 2^(P-1) + 0.5; then clamp to
 * [0, 2^P - 1] and truncate.  Coefficients with k >= N or h >= N are not read.  Against the textbook form -- (N / 8) x
 * the orthonormal N-point 2-D IDCT of the top-left N x N dequantised coefficients, plus level, clamped, truncated -- a
 * sample differs by at most one level, and only where that value lies at an integer boundary.
 *
 * Interleave and colour: Planar.interleaved(cosite:) and Rectangular.unpack(as:) (decode.swift:4182-4276,
 * jpeg.swift:343-354, 441-478) unchanged, at the image size (W', H'), with the padded plane's edge last = N units - 1 in
 * the place of 8 units - 1: direct planes, the centred and cosited (a, b, c), the fraction clamp, the two-step bilinear
 * sum, .rounded(), YCbCr.rgb and the clamping byte conversion are the reference's.  Pixel W' - 1 never indexes past
 * N units - 1 where units = ceil(W f / (8 s)):  W' - 1 < W N / 8, so its cosited index f (W' - 1) / s < N W f / (8 s) <=
 * N units; the centred index (f - s + 2 f t) / (2 s) = f t / s + (f - s) / (2 s) <= f t / s is no larger (f <= s).  A
 * direct plane reads sample t <= W' - 1 <= N units - 1 because 8 units >= W.  (Planes given with other units must cover
 * the scaled image in the same sense, else EINVAL.)
 *
 * denom == 1 is jpeg_amd_decode_batch itself: the same call, the same bytes.  Everything else follows
 * jpeg_amd_decode_batch: 8-bit only (else ENOSUP), 1 or 3 planes, at most 65 535 images, n_images == 0 is OK; everything
 * is validated before anything is enqueued and on EINVAL nothing is written.  Any other denom is EINVAL.
 * Image i at d_pixels + i * pixel_stride: H' rows of 3 W' bytes; pixel_stride >= 3 W' H' (any value, 0 included, when
 * n_images == 1); bytes in the stride gaps are left alone.
 * Cost: the layouts of the fused decode (y8; ycc8 with full-factor luma and chroma at 1x or 2x per axis, centred) take
 * one launch that fetches only the head of each block (half of it at denom 2, 16 bytes at denom 4, 2 bytes at denom 8).
 * Other layouts (cosited, factors 3 or 4, ...) transform every plane into context scratch, padded to whole blocks by edge
 * replication, and run the staged interleave kernel under jpeg_amd_scaled_layout's layout. */
int jpeg_amd_decode_scaled_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, int n_images,
                                 const int16_t *const d_coef[], const size_t coef_stride[],
                                 const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                 int cosited, jpeg_amd_color color, int denom,
                                 uint8_t *d_pixels, size_t pixel_stride);
/* single image, host tables */
int jpeg_amd_decode_scaled(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, const int16_t *const d_coef[],
                           const uint16_t *h_quanta, int ntables, int cosited, jpeg_amd_color color, int denom,
                           uint8_t *d_pixels);
/* Host only.  The layout of the scaled image as the staged calls see it: (W', H'), the same precision, factors, scale and
 * tables, units ceil(N units / 8) -- the scaled planes padded to whole 8 x 8 blocks.  Padded by EDGE REPLICATION (sample
 * (x, y) of the padding = sample (min(x, N units_x - 1), min(y, N units_y - 1))) they give, through
 * jpeg_amd_planar_interleaved and jpeg_amd_rectangular_unpack under this layout, the contract's pixels: replication makes
 * min(i + 1, 8 units' - 1) read the value min(i + 1, N units - 1) reads.  EINVAL for a denom not in {1, 2, 4, 8}. */
int jpeg_amd_scaled_layout(const jpeg_amd_layout *in, int denom, jpeg_amd_layout *out);
/* The staged form of the transform alone (single image, host tables, any precision): d_planes[p] is the scaled plane p
 * as uint16 [8 units_y'][8 units_x'] under jpeg_amd_scaled_layout's units, edge-replicated as described there. */
int jpeg_amd_spectral_idct_scaled(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, const int16_t *const d_coef[],
                                  const uint16_t *h_quanta, int ntables, int denom, uint16_t *const d_planes[]);

/* ---- view decode: a rectangle of the scaled image, a denominator and a rectangle per image ----------
 * A view is a denominator and a rectangle in pixels of the image that denominator gives. */
typedef struct jpeg_amd_view {
    int32_t denom;
    jpeg_amd_region region;
} jpeg_amd_view;

/* Image i of the output is THE IMAGE THAT jpeg_amd_decode_scaled_batch DEFINES FOR views[i].denom, CROPPED TO
 * views[i].region, bit for bit.  Nothing is defined here arithmetically: the scaled contract above (tables, reduced
 * butterflies, last = N units - 1, the reference's interleave and colour stage at size (W', H')) is the contract.  For
 * denom == 1 that image is jpeg_amd_decode_batch's, and the view is exactly a region of jpeg_amd_decode_region_batch.
 *
 * denom in {1, 2, 4, 8}, N = 8 / denom, else EINVAL.  The region is in pixels of the scaled image (W', H') =
 * (ceil(W N / 8), ceil(H N / 8)), any alignment: x, y >= 0, width, height > 0, x + width <= W', y + height <= H', else
 * EINVAL.  Output image i at d_pixels + i * pixel_stride: region.height rows of region.width * 3 bytes, no padding between
 * rows; pixel_stride >= 3 * width_i * height_i for every i (any value, 0 included, when n_images == 1); bytes in the stride
 * gaps are left alone.  h_views is a HOST array of n_images views, any mix of denominators; the call copies it before it
 * returns, as h_regions.  Every view is validated before anything is enqueued: on EINVAL nothing is written and the context
 * stays usable.  Everything else as jpeg_amd_decode_batch: 8-bit only (else ENOSUP), 1 or 3 planes, at most 65 535 images,
 * n_images == 0 is OK.
 * Cost: for the layouts of the fused decode (y8; ycc8 with full-factor luma and chroma at 1x or 2x per axis, centred) one
 * launch per distinct denominator of the call, four at most, each over the images of that denominator; a view reads only
 * the heads of the blocks of its window (jpeg_amd_view_window) and writes only its pixels.  Other layouts (cosited, factors
 * 3 or 4, ...) decode the WHOLE scaled images into context scratch -- run by run of consecutive images of one denominator,
 * in chunks of at most 1 GiB -- and crop: correct, but as costly as the scaled decode of every image.  A call whose views
 * are all whole images at one denominator is jpeg_amd_decode_scaled_batch (jpeg_amd_decode_batch at denominator 1); one
 * whose denominators are all 1 is jpeg_amd_decode_region_batch. */
int jpeg_amd_decode_view_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, int n_images,
                               const int16_t *const d_coef[], const size_t coef_stride[],
                               const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                               int cosited, jpeg_amd_color color, const jpeg_amd_view *h_views,
                               uint8_t *d_pixels, size_t pixel_stride);
/* single image, host tables */
int jpeg_amd_decode_view(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, const int16_t *const d_coef[],
                         const uint16_t *h_quanta, int ntables, int cosited, jpeg_amd_color color,
                         const jpeg_amd_view *view, uint8_t *d_pixels);
/* Host only.  jpeg_amd_region_window for a view: windows[p] (in BLOCKS of plane p, for p < nplanes; the rest are zeroed)
 * is the smallest block rectangle that holds every sample of the scaled plane p -- N x N per block -- that the contract
 * reads for some pixel of `region` of the image at `denom`: N in the place of 8, N units - 1 as the padded edge,
 * zero-weight neighbours included.  At denom 1 it is jpeg_amd_region_window.  EINVAL for a denom not in {1, 2, 4, 8}, a
 * region outside (W', H'), or a layout whose planes do not cover the scaled image. */
int jpeg_amd_view_window(const jpeg_amd_layout *layout, int cosited, int denom, const jpeg_amd_region *region,
                         jpeg_amd_region windows[JPEG_AMD_MAX_PLANES]);
/* Host only.  The smallest rectangle of the image at `denom` that covers `source_region`, a rectangle in pixels of the
 * full-size image (scaled pixel x' stands for the source pixels [8 x' / N, 8 (x' + 1) / N)):  x' = floor(x N / 8),
 * x1' = min(W', ceil((x + width) N / 8)), the same for y.  EINVAL for a source rectangle outside the image. */
int jpeg_amd_view_of_source(const jpeg_amd_layout *layout, int denom, const jpeg_amd_region *source_region,
                            jpeg_amd_region *region);
/* Host only, pure.  The largest denom in {8, 4, 2, 1} with floor(src_w N / 8) >= want_w and floor(src_h N / 8) >= want_h
 * (N = 8 / denom), 1 if none: the cheapest reduction of a src_w x src_h source rectangle that still needs no upscaling
 * to reach want_w x want_h. */
int jpeg_amd_view_denom(int32_t src_w, int32_t src_h, int32_t want_w, int32_t want_h);

/* ---- resized decode: views resampled to one fixed size ------------------------------------------------
 * The reference has no resize; this is the conventional bilinear filter with half-pixel centres.  THE CONTRACT (the one
 * statement of it), every statement ONE binary32 operation, nothing contracted:
 *
 * A source image is w x h pixels of 3 bytes, the target out_w x out_h.  Per axis, here x for output column j:
 *   kx = (float)w / (float)out_w               divided ON THE HOST, handed to the kernel per image: the kernel holds no
 *                                              division and nothing depends on a device division mode
 *   sx = ((float)j + 0.5f) * kx - 0.5f;  sx = max(sx, 0.0f)
 *   x0 = min((int)sx, w - 1);  x1 = min(x0 + 1, w - 1);  fx = sx - (float)x0
 * and y0, y1, fy from ky = (float)h / (float)out_h and the output row likewise.  Per channel, with a, b, c, d the bytes at
 * (y0, x0), (y0, x1), (y1, x0), (y1, x1) converted to float -- the horizontal pass first, then the vertical pass:
 *   top = a + fx * (b - a);  bot = c + fx * (d - c);  v = top + fy * (bot - top)
 *   out = (uint8)(int)(min(max(v, 0.0f), 255.0f) + 0.5f)
 * There is no antialiasing filter in these calls ("antialiased resample" below has them with one): with a denominator
 * from jpeg_amd_view_denom what is left to reduce is below 2 per axis unless the source is more than 8 times the target.
 * out_w == w and out_h == h give the source bytes (sx = j, fx = 0).
 * Upscaling is the same formula. */
typedef struct jpeg_amd_extent {
    int32_t width, height;
} jpeg_amd_extent;

/* The resample alone, pixels to pixels, one launch.  Source image i is h_extents[i].height rows of 3 * width bytes, no
 * padding between rows, at d_src + i * src_stride; output image i is out_h rows of 3 * out_w bytes at d_dst + i * dst_stride.
 * src_stride >= 3 * width_i * height_i for every i and dst_stride >= 3 * out_w * out_h (any value, 0 included, when
 * n_images == 1); bytes in the stride gaps are left alone.  The source and the output must not overlap.  h_extents is a HOST
 * array of n_images extents; the call copies it before it returns.  Everything is validated before anything is enqueued: on
 * EINVAL -- out_w or out_h < 1 or above 2^30, a width or height < 1, a stride that is too small, more than 65 535 images, a
 * null pointer -- nothing is written and the context stays usable.  n_images == 0 is OK. */
int jpeg_amd_resize_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                          const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, uint8_t *d_dst, size_t dst_stride);

/* Image i of the output is THE IMAGE THAT jpeg_amd_decode_view_batch DEFINES FOR h_views[i], RESAMPLED to out_w x out_h by
 * the contract above; nothing else is defined here arithmetically.  Output and its stride as in jpeg_amd_resize_batch,
 * every other argument as in jpeg_amd_decode_view_batch, and whatever either refuses is refused here -- before anything is
 * enqueued, nothing written, the context usable (8-bit only, else ENOSUP; n_images == 0 is OK).
 * Cost: jpeg_amd_decode_view_batch, as it stands, into a buffer of the context (each view compact, the views of a chunk at
 * a stride of the chunk's largest, chunks of consecutive images of at most 1 GiB), then ONE resample launch per chunk.
 * Every layout of the view call works, its fallback layouts included. */
int jpeg_amd_decode_resized_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, int n_images,
                                  const int16_t *const d_coef[], const size_t coef_stride[],
                                  const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                  int cosited, jpeg_amd_color color, const jpeg_amd_view *h_views,
                                  int32_t out_w, int32_t out_h, uint8_t *d_pixels, size_t pixel_stride);
/* single image, host tables */
int jpeg_amd_decode_resized(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, const int16_t *const d_coef[],
                            const uint16_t *h_quanta, int ntables, int cosited, jpeg_amd_color color,
                            const jpeg_amd_view *view, int32_t out_w, int32_t out_h, uint8_t *d_pixels);

/* ---- tensor output: resized views as normalised float tensors (CHW / HWC, horizontal flip) ------------
 * The tail every training loop runs on a resized batch -- flip, permute, convert, subtract mean, divide by std, cast -- in
 * the resample's own launch.  THE CONTRACT (the one statement of it): the tensor output defines no resample arithmetic of
 * its own.  Let u(i, y, x, c) be the byte that jpeg_amd_resize_batch (or jpeg_amd_decode_resized_batch) defines for image i,
 * row y, column x, channel c.  The element stored for (i, c, y, x) is
 *   xs = flip[i] ? out_w - 1 - x : x            the RESAMPLED image mirrored; NOT a mirrored source rectangle
 *   t  = (float)u(i, y, xs, c) - mean[c]        one binary32 operation
 *   v  = t * scale[c]                           one binary32 operation, nothing contracted
 *   element = v                                 JPEG_AMD_F32
 *           | v rounded to binary16             JPEG_AMD_F16, round to nearest even
 *           | v rounded to bfloat16             JPEG_AMD_BF16, round to nearest even: with `bits` the binary32 pattern of v,
 *                                               (bits + 0x7fff + ((bits >> 16) & 1)) >> 16
 * mean is in BYTE units (255 * 0.485, say) and scale is what the caller wants multiplied (1 / (255 * 0.229)), both rounded
 * to binary32 by the caller: the kernel holds no division.  There are always three channels, like the byte calls (grey
 * layouts give three equal bytes there), and `color` passes through unchanged.
 * Layouts, in ELEMENTS, image i at d_dst + i * dst_stride elements:
 *   JPEG_AMD_TENSOR_HWC   element (y * out_w + x) * 3 + c
 *   JPEG_AMD_TENSOR_CHW   element (c * out_h + y) * out_w + x
 * Elements in the stride gaps are left alone. */
enum { JPEG_AMD_F32 = 0, JPEG_AMD_F16 = 1, JPEG_AMD_BF16 = 2 };
enum { JPEG_AMD_TENSOR_HWC = 0, JPEG_AMD_TENSOR_CHW = 1 };
typedef struct jpeg_amd_tensor_spec {
    int32_t dtype;    /* JPEG_AMD_F32 | JPEG_AMD_F16 | JPEG_AMD_BF16 */
    int32_t layout;   /* JPEG_AMD_TENSOR_HWC | JPEG_AMD_TENSOR_CHW */
    float mean[3], scale[3];
} jpeg_amd_tensor_spec;

/* Host only, pure.  *elem_bytes = the element size (4, 2, 2) and *image_elems = 3 * out_w * out_h (either pointer may be
 * NULL).  EINVAL for a NULL spec, an unknown dtype or layout, a mean or scale that is not finite, or an out_w / out_h that
 * jpeg_amd_resize_batch refuses. */
int jpeg_amd_tensor_extent(const jpeg_amd_tensor_spec *spec, int32_t out_w, int32_t out_h, size_t *elem_bytes,
                           size_t *image_elems);
/* The resample and the output stage alone, one launch.  Sources, src_stride, h_extents, out_w and out_h as in
 * jpeg_amd_resize_batch.  h_flip: a HOST array of n_images bytes, nonzero = mirror image i; NULL = none.  spec and h_flip are
 * copied before the call returns.  d_dst is aligned to the element size; dst_stride, in elements, >= 3 * out_w * out_h (any
 * value, 0 included, when n_images == 1).  Everything is validated before anything is enqueued: on EINVAL -- what
 * jpeg_amd_tensor_extent refuses, a misaligned d_dst, a stride that is too small, a null pointer, and whatever
 * jpeg_amd_resize_batch refuses -- nothing is written and the context stays usable.  n_images == 0 is OK. */
int jpeg_amd_resize_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                 const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h,
                                 const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst, size_t dst_stride);
/* Views to tensor: every argument up to out_h as in jpeg_amd_decode_resized_batch, spec, h_flip, d_dst and dst_stride as
 * above; whatever either refuses is refused here, before anything is enqueued.
 * Cost: exactly jpeg_amd_decode_resized_batch's route -- jpeg_amd_decode_view_batch, as it stands, into the context's
 * buffer in chunks of at most 1 GiB, then ONE launch per chunk that resamples and writes the elements.  Every layout of the
 * view call works, its fallback layouts included. */
int jpeg_amd_decode_tensor_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, int n_images,
                                 const int16_t *const d_coef[], const size_t coef_stride[],
                                 const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                 int cosited, jpeg_amd_color color, const jpeg_amd_view *h_views,
                                 int32_t out_w, int32_t out_h, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                 void *d_dst, size_t dst_stride);
/* single image, host tables; flip: nonzero = mirrored */
int jpeg_amd_decode_tensor(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, const int16_t *const d_coef[],
                           const uint16_t *h_quanta, int ntables, int cosited, jpeg_amd_color color,
                           const jpeg_amd_view *view, int32_t out_w, int32_t out_h, const jpeg_amd_tensor_spec *spec,
                           int flip, void *d_dst);

/* ---- mixed calls: views of images of different sizes and layouts in one call -----------------------------
 * What a data loader has: n files of n sizes, some 4:2:0, some 4:4:4, some grey, to one tensor.  The view, resized and
 * tensor calls above take one layout per call; these take one per IMAGE. */
typedef struct jpeg_amd_image {          /* one image of a mixed call */
    jpeg_amd_layout layout;              /* its own geometry */
    const int16_t  *d_coef[JPEG_AMD_MAX_PLANES];
    const uint16_t *d_quanta;            /* device, [ntables][64], zigzag */
    int32_t         ntables;
} jpeg_amd_image;

/* THE CONTRACT (the one statement of it): image i of the output is EXACTLY WHAT THE UNIFORM CALL WRITES FOR IMAGE i WHEN
 * CALLED ON IT ALONE, bit for bit -- jpeg_amd_decode_view_batch, jpeg_amd_decode_resized_batch or
 * jpeg_amd_decode_tensor_batch with n_images = 1, h_images[i].layout, its planes (any strides), its tables (ntables of
 * them), h_views[i] and, for the tensor call, h_flip[i].  No arithmetic is defined here.
 *
 * h_images and h_views are HOST arrays of n_images elements; the call copies them before it returns (h_flip as in
 * jpeg_amd_resize_tensor_batch: NULL = no image mirrored).  cosited and color hold for every image.  Output placement and
 * strides are the uniform calls': for the view call image i is at d_pixels + i * pixel_stride, region.height rows of
 * region.width * 3 bytes, and pixel_stride >= 3 * width_i * height_i for every i (any value when n_images == 1); for the
 * resized and the tensor call as in jpeg_amd_decode_resized_batch and jpeg_amd_decode_tensor_batch.  Bytes in the stride
 * gaps are left alone.
 *
 * Everything is judged before anything is enqueued, the context last.  Each image's layout, planes, tables and view are
 * checked against ITS OWN layout, and the status is the one the uniform call gives for the first offending image in index
 * order: EINVAL for a view outside that image's scaled size, a null plane pointer, a denominator not in {1, 2, 4, 8}, an
 * ntables at or below a plane's qi, a stride that is too small; ENOSUP for an image that is not 8-bit (one 12-bit image
 * refuses the whole call).  EINVAL also for n_images < 0 or above 65 535, null h_images or h_views, and a launch whose
 * summed workgroups do not fit a grid.  After a refused call nothing has been written and the context is usable.
 * n_images == 0 is OK.
 *
 * Cost: the images whose layout the fused decode takes (y8; ycc8 with full-factor luma and chroma at 1x or 2x per axis,
 * centred) are grouped by (N = 8 / denom, 1 or 3 planes): at most EIGHT launches of the tile kernel, each over the images
 * of its group whatever their sizes and whatever their mix of 4:4:4, 4:2:2, 4:4:0 and 4:2:0, behind ONE host-to-device
 * copy of the per-image records.  The mixed calls ALWAYS take the tile kernel for those images: a call of whole images, or
 * of denominators that are all 1, has no shortcut into the whole-image or the region kernels as the uniform view call has;
 * for such a batch of one geometry the uniform calls are the faster ones.  Every other image (cosited calls, factors 3 or
 * 4, chroma not at 1x or 2x) goes through the uniform call ONE IMAGE AT A TIME: correct, and as costly as that sounds.
 * The resized and the tensor call follow jpeg_amd_decode_resized_batch's route: chunks of consecutive images of at most
 * 1 GiB of compact views in a buffer of the context, per chunk the mixed view decode and then ONE resample launch. */
int jpeg_amd_decode_view_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                               jpeg_amd_color color, const jpeg_amd_view *h_views, uint8_t *d_pixels, size_t pixel_stride);
int jpeg_amd_decode_resized_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                  jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                  uint8_t *d_pixels, size_t pixel_stride);
int jpeg_amd_decode_tensor_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                 jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                 const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst, size_t dst_stride);

/* ---- antialiased resample: a second filter for the resized, tensor and mixed calls ----------------------
 * The bilinear filter of "resized decode" reads two source samples per axis whatever the reduction, so it aliases as soon as
 * a source is larger than the target.  This is the triangle filter WIDENED BY THE SCALE FACTOR, the filter that
 * torch.nn.functional.interpolate(mode="bilinear", antialias=True) and PIL's BILINEAR compute.  THE CONTRACT (the one
 * statement of it), every statement ONE binary32 operation, nothing contracted:
 *
 * Per axis, for n source samples, n_out outputs and output index j:
 *   k  = (float)n / (float)n_out          on the host, per image, as in "resized decode"
 *   s  = max(k, 1.0f)                     on the host
 *   r  = 1.0f / s                         on the host: the kernel is handed k, s and r
 *   c  = ((float)j + 0.5f) * k
 *   lo = max((int)((c - s) + 0.5f), 0)
 *   hi = min((int)((c + s) + 0.5f), n)    taps t = lo .. hi - 1, at least one
 *   u_t = (((float)t - c) + 0.5f) * r
 *   w_t = max(1.0f - fabsf(u_t), 0.0f)
 *   total = w_lo + w_(lo+1) + ...         left to right, ascending t
 *   W_t = w_t / total                     IEEE-754 correctly rounded binary32 division
 * The division happens once per output column and once per output row of a tile of the kernel, never per pixel; the library
 * is built without fast-math and with the compiler's default, correctly rounded, division.
 * Per channel, with p(y, t) the source byte converted to float -- the horizontal pass first, its result kept as a float:
 *   h(y) = (...((0.0f + W_lo * p(y, lo)) + W_(lo+1) * p(y, lo+1)) + ...)      x taps ascending; a product, then a sum
 *   v    = (...((0.0f + Wy_lo * h(lo)) + Wy_(lo+1) * h(lo+1)) + ...)          y taps ascending
 *   out  = (uint8)(int)(min(max(v, 0.0f), 255.0f) + 0.5f)
 * out_w == w and out_h == h give the source bytes (the weights are 1 and 0).  Upscaling is the same formula with s = 1.
 * The tensor output is unchanged: with u(i, y, x, c) this byte, "tensor output" applies as it stands -- the flip of the
 * RESAMPLED image, minus mean, times scale, one rounding.
 *
 * THE LIMIT.  s <= 16 per axis keeps the taps of an output at 33 or fewer (the interval has length 2 s).  An image whose kx
 * or ky, as computed above in binary32, exceeds 16.0f makes the whole call JPEG_AMD_ENOSUP: after everything the bilinear
 * form of the same call refuses and before the context is touched, by the first offending image in index order; nothing is
 * written and the context stays usable.  Behind a denominator of 8 that is a reduction of 128 per axis.
 *
 * THE CALLS.  Each takes exactly the arguments of the call it is named after, with `filter` directly after out_h.
 * JPEG_AMD_FILTER_BILINEAR is, bit for bit and status for status, that call.  Any other value of `filter` than the two below
 * and JPEG_AMD_FILTER_BICUBIC ("bicubic resample") is EINVAL.  There are no single-image forms: n_images == 1 serves.
 * Cost: the route of the call it is named after, with the antialiasing kernel in the place of the bilinear one.  That
 * kernel reads every source pixel of an output tile's footprint once per tile (the bilinear one reads four per output
 * pixel), so its time grows with kx ky. */
enum { JPEG_AMD_FILTER_BILINEAR = 0, JPEG_AMD_FILTER_ANTIALIAS = 1 };

int jpeg_amd_resize_filter_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                 const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, int filter,
                                 uint8_t *d_dst, size_t dst_stride);
int jpeg_amd_resize_filter_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                        const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, int filter,
                                        const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst,
                                        size_t dst_stride);
int jpeg_amd_decode_resized_filter_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, int n_images,
                                         const int16_t *const d_coef[], const size_t coef_stride[],
                                         const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                         int cosited, jpeg_amd_color color, const jpeg_amd_view *h_views,
                                         int32_t out_w, int32_t out_h, int filter, uint8_t *d_pixels, size_t pixel_stride);
int jpeg_amd_decode_tensor_filter_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, int n_images,
                                        const int16_t *const d_coef[], const size_t coef_stride[],
                                        const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                        int cosited, jpeg_amd_color color, const jpeg_amd_view *h_views,
                                        int32_t out_w, int32_t out_h, int filter, const jpeg_amd_tensor_spec *spec,
                                        const uint8_t *h_flip, void *d_dst, size_t dst_stride);
int jpeg_amd_decode_resized_filter_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                         jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                         int filter, uint8_t *d_pixels, size_t pixel_stride);
int jpeg_amd_decode_tensor_filter_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                        jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                        int filter, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst,
                                        size_t dst_stride);

/* ---- bicubic resample: a third filter for the same calls ---------------------------------------------------
 * The filter most published ImageNet recipes resize with.  This is the Keys cubic with a = -0.5, WIDENED BY THE SCALE
 * FACTOR, clipped at the image edge and renormalised: the filter of torch.nn.functional.interpolate(mode="bicubic",
 * antialias=True) and of torchvision's Resize(BICUBIC, antialias=True) on tensors.  (torch's bicubic WITHOUT antialias uses
 * a = -0.75 and four fixed taps: a different filter, which this library does not offer.  PIL's BICUBIC is this kernel too,
 * but PIL rounds to bytes between its passes, so its bytes differ -- by up to 22 levels on random content.)  THE CONTRACT
 * (the one statement of it), every statement ONE binary32 operation, nothing contracted:
 *
 * Per axis, for n source samples, n_out outputs and output index j:
 *   k  = (float)n / (float)n_out          on the host, per image
 *   s  = max(k, 1.0f)                     on the host
 *   r  = 1.0f / s                         on the host: the kernel is handed k, s and r, as in "antialiased resample"
 *   p  = 2.0f * s                         (exact) the half-width of the support
 *   c  = ((float)j + 0.5f) * k
 *   lo = max((int)((c - p) + 0.5f), 0)
 *   hi = min((int)((c + p) + 0.5f), n)    taps t = lo .. hi - 1, at least one
 *   u_t = (((float)t - c) + 0.5f) * r
 *   x   = fabsf(u_t)
 *   x < 1:  w_t = ((1.5f * x - 2.5f) * x) * x + 1.0f                     five operations, in this order
 *   x < 2:  w_t = ((((x - 5.0f) * x + 8.0f) * x) - 4.0f) * -0.5f          six operations, in this order
 *   else:   w_t = 0.0f
 *   total = w_lo + w_(lo+1) + ...         left to right, ascending t; positive (0.5 is the least a clipped edge leaves)
 *   W_t = w_t / total                     IEEE-754 correctly rounded binary32 division
 * The two passes and the conversion to a byte are those of "antialiased resample", word for word: the horizontal pass first,
 * its result kept as a float; then the vertical pass; a product and then a sum per tap, ascending; then
 *   out = (uint8)(int)(min(max(v, 0.0f), 255.0f) + 0.5f)
 * The weights are negative in the lobes (1 < x < 2), so v leaves 0 ... 255 at hard edges and the clamp is live here.
 * out_w == w and out_h == h give the source bytes (u is an integer: the weights are exactly 1 and 0).  The tensor output, the
 * flip and the orientation are unchanged: they act on this byte.
 *
 * THE LIMIT.  The support is 4 s wide, so an output reads at most 4 s + 1 taps; s <= 8 per axis keeps them at 33 or fewer.
 * An image whose kx or ky, as computed above in binary32, exceeds 8.0f makes the whole call JPEG_AMD_ENOSUP, placed and
 * ordered exactly as the limit of "antialiased resample" is: after everything the bilinear form of the same call refuses and
 * before the context is touched, by the first offending image in index order; nothing is written and the context stays
 * usable.  k == 8.0f exactly is accepted (32 taps).  Behind a denominator of 8 that is a reduction of 64 per axis.
 *
 * THE CALLS.  Every call that takes `filter` -- the six *_filter_* calls above, the *_oriented_* calls and the file calls
 * below -- takes this value; there is no new entry point.  The value 2 stays EINVAL.
 * Cost: the antialiasing kernel's route and walk with tables twice as wide: about twice its taps per output at k >= 1
 * (four per axis instead of two at k <= 1). */
enum { JPEG_AMD_FILTER_BICUBIC = 3 };

/* ---- tensor sources: float and uint8 tensors (CHW / HWC) into the encoders --------------------------------
 * The mirror of "tensor output": what a framework holds -- a model's float CHW output in 0 ... 1 or in normalised units,
 * torchvision's uint8 [3, H, W] -- turned into the encoders' tight uint8 [H][W][3] rows by ONE launch, in the place of the
 * mul, add, clamp, round, cast, permute, contiguous a caller runs otherwise.  THE CONTRACT (the one statement of it): the
 * byte u(i, y, x, c) of image i is made from the element e of (i, c, y, x); every line is ONE binary32 operation, nothing
 * contracted:
 *   f = e as binary32                 JPEG_AMD_F16 and JPEG_AMD_BF16 convert exactly; subnormal elements are numbers (no
 *                                     flushing)
 *   p = f * scale[c]
 *   s = p + offset[c]
 *   b = fminf(fmaxf(s, 0), 255)       fmaxf / fminf return the other operand when one is NaN: NaN -> 0, +Inf -> 255,
 *                                     -Inf -> 0
 *   u = (uint8_t)(int)(b + 0.5f)      the sum rounded to binary32, then truncated: the conversion of "resized decode"
 *   JPEG_AMD_U8:  u = e;  scale and offset are not read
 * scale and offset are in BYTE units (255 * std and 255 * mean invert "tensor output"; 255 and 0 take 0 ... 1), both rounded
 * to binary32 by the caller: the kernel holds no division.  There are always three channels, and `color` passes through to
 * the encoder unchanged.  Element indices of `layout` are those of "tensor output" with (w, h) for (out_w, out_h); image i
 * is at d_src + i * src_stride ELEMENTS.
 * The encode and compress calls below define no encoder arithmetic: their coefficients and files are, bit for bit, those of
 * jpeg_amd_encode_batch / jpeg_amd_compress_batch_device on the bytes u. */
enum { JPEG_AMD_U8 = 3 };   /* sources only; jpeg_amd_tensor_extent keeps refusing it */
typedef struct jpeg_amd_tensor_source {
    int32_t dtype;    /* JPEG_AMD_F32 | JPEG_AMD_F16 | JPEG_AMD_BF16 | JPEG_AMD_U8 */
    int32_t layout;   /* JPEG_AMD_TENSOR_HWC | JPEG_AMD_TENSOR_CHW, element indices as in "tensor output" */
    float scale[3], offset[3];
} jpeg_amd_tensor_source;

/* Host only, pure.  *elem_bytes = the element size (4, 2, 2, 1) and *image_elems = 3 * w * h (either pointer may be NULL).
 * EINVAL for a NULL source, an unknown dtype or layout, a scale or offset that is not finite under a float dtype, or a w or
 * h outside 1 ... 65 535. */
int jpeg_amd_tensor_source_extent(const jpeg_amd_tensor_source *src, int32_t w, int32_t h, size_t *elem_bytes,
                                  size_t *image_elems);
/* The front alone, one launch: n_images sources of w x h to bytes, image i at d_pixels + i * pixel_stride (h rows of 3 w
 * bytes; pixel_stride in bytes, 0 = 3 w h).  d_src is aligned to the element size; src_stride (elements) and pixel_stride
 * >= 3 w h (any value when n_images == 1); bytes in the stride gaps are left alone; the source and the output must not
 * overlap.  src is copied before the call returns.  At most 65 535 images, n_images == 0 is OK.  Everything is validated
 * before anything is enqueued: on EINVAL -- what jpeg_amd_tensor_source_extent refuses, a misaligned d_src, a stride that
 * is too small, a null pointer -- nothing is written and the context stays usable. */
int jpeg_amd_tensor_pixels_batch(jpeg_amd_ctx *ctx, int n_images, const void *d_src, size_t src_stride, int32_t w, int32_t h,
                                 const jpeg_amd_tensor_source *src, uint8_t *d_pixels, size_t pixel_stride);
/* jpeg_amd_encode_batch with (d_src, src_stride, src) in the place of (d_pixels, pixel_stride); the extent is the layout's.
 * Whatever jpeg_amd_encode_batch refuses is refused first, with its status, then what jpeg_amd_tensor_pixels_batch refuses;
 * nothing is enqueued on a refusal.
 * Cost: chunks of consecutive images of at most 1 GiB of bytes in a buffer of the context, per chunk ONE front launch and
 * then jpeg_amd_encode_batch as it stands -- every layout it takes works, its staged layouts included.  A JPEG_AMD_U8,
 * JPEG_AMD_TENSOR_HWC source IS jpeg_amd_encode_batch on d_src: no launch, no buffer. */
int jpeg_amd_encode_tensor_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, int n_images, const void *d_src,
                                 size_t src_stride, const jpeg_amd_tensor_source *src, jpeg_amd_color color,
                                 const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                 int16_t *const d_coef[], const size_t coef_stride[]);
/* single image, host tables */
int jpeg_amd_encode_tensor(jpeg_amd_ctx *ctx, const jpeg_amd_layout *layout, const void *d_src,
                           const jpeg_amd_tensor_source *src, jpeg_amd_color color, const uint16_t *h_quanta, int ntables,
                           int16_t *const d_coef[]);
/* jpeg_amd_compress_batch_device with (d_src, src_stride, src) in the place of (d_pixels, pixel_stride); src_stride in
 * elements, 0 = 3 W H.  Whatever that call refuses is refused first, then the source.  The front launch writes each
 * chunk's bytes into the pipeline's device slot; everything behind it is that call's. */
int jpeg_amd_compress_tensor_batch_device(jpeg_amd_ctx *ctx, jpeg_amd_frame_info *frame, const void *d_src,
                            size_t src_stride, const jpeg_amd_tensor_source *src, int n_images, jpeg_amd_color color,
                            const int32_t *quanta_key, const uint16_t *h_quanta,
                            const int32_t *h_quanta_keys, int ntables, const jpeg_amd_scan *scans,
                            int nscans, const jpeg_amd_metadata *metadata, int nmetadata, int nthreads,
                            uint8_t *h_out, size_t out_stride, size_t nbytes[]);

/* ---- spectral reduce: a Spectral at 1/2, 1/4 or 1/8 size, coefficients in and coefficients out ----------
 * JPEG in, smaller JPEG out, without pixels in between: no interleave, no colour conversion and no second generation of
 * chroma rounding, so every layout, plane count and precision is served alike.  It composes two contracts that are stated
 * elsewhere and defines no arithmetic of its own.  THE CONTRACT (the one statement of it):
 *
 * denom in {2, 4, 8}, N = 8 / denom.  Any other value is EINVAL -- 1 included: requantising at full size is
 * jpeg_amd_spectral_transform's job.
 *
 * Scaled samples.  For plane p of units (ux, uy) and table Q_in, S_p is the N uy x N ux sample array that the
 * scaled-decode contract above defines: the table q_N, the reduced butterflies, the two passes, clamp to [0, 2^P - 1] and
 * truncate at the layout's precision P.  Coefficients with k >= N or h >= N are not read.
 *
 * Output geometry (jpeg_amd_reduce_layout).  (W', H') = (ceil(W N / 8), ceil(H N / 8)); precision, factors, scale and qi
 * are the input's; the units are recomputed exactly as jpeg_amd_layout_units does for (W', H') -- what any reader of the
 * output file derives from its header.  Where every factor divides the scale these are jpeg_amd_scaled_layout's
 * ceil(N units / 8); for a factor that does not divide the scale they can be one larger (factor 3 in scale 4, width 21,
 * N = 4: 2 against 1).  The replication rule covers both.
 *
 * Output samples.  Plane p of the output is 8 uy' x 8 ux' samples; sample (x, y) is S_p(min(x, N ux - 1), min(y, N uy - 1)):
 * edge replication, the rule jpeg_amd_scaled_layout documents.
 *
 * Output coefficients.  Spectral.Plane.fdct(_:quanta:precision:) (encode.swift:199-248) of that plane with table Q_out:
 * load(limit:), fdct8x8, the x8 modulated table, the quotient rounded half away from zero -- exactly what
 * jpeg_amd_planar_fdct computes (oracle/: fdct_plane).  Q_out is given per table index like Q_in; NULL means Q_in.
 *
 * The quantiser is the literal binary32 division of the staged FDCT kernel (the only other form the contract admits is the
 * fused encoder's reciprocal-plus-correction inside the range tools/verify_div16.hip proved: every 16-bit divisor,
 * numerators below 2^25).  A quotient that does not fit int16 behaves as in jpeg_amd_planar_fdct; nothing new is defined
 * for it.  A zero in a HOST-supplied output table (NULL = the input tables) is EINVAL; the batch entry takes DEVICE tables,
 * like jpeg_amd_encode_batch, and validates what that call validates.
 *
 * Cost: one launch for every plane of every image; it reads only the block heads the scaled decode reads (half a block at
 * denom 2, 16 bytes at denom 4, 2 bytes at denom 8) and writes 1/4, 1/16 or 1/64 of the input's bytes. */

/* Host only.  The output geometry above; EINVAL for a denom not in {2, 4, 8} or an invalid layout. */
int jpeg_amd_reduce_layout(const jpeg_amd_layout *in, int denom, jpeg_amd_layout *out);
/* n_images images of layout in_layout: image i of plane p reads d_coef_in[p] + i * in_stride[p] and writes d_coef_out[p] +
 * i * out_stride[p] (int16 elements; the output planes are sized by jpeg_amd_reduce_layout; int16 elements in the stride gaps
 * are left alone).  Plane pointers are multiples of 16 bytes and, for more than one image, strides multiples of 8 elements, else
 * EINVAL: every block starts on a 16-byte boundary.  Every plane of in_layout has at least one block.  d_quanta: DEVICE tables [..][ntables][64], image i at
 * i * quanta_stride, plane p uses table in_layout->qi[p]; d_quanta_out: NULL = d_quanta, else the output tables, same layout
 * and strides.  At most 65 535 images, n_images == 0 is OK.  Everything is validated before anything is enqueued: on EINVAL
 * nothing is written and the context stays usable.  Asynchronous on the ctx stream. */
int jpeg_amd_spectral_reduce_batch(jpeg_amd_ctx *ctx, const jpeg_amd_layout *in_layout, int n_images, int denom,
                                   const int16_t *const d_coef_in[], const size_t in_stride[],
                                   const uint16_t *d_quanta, size_t quanta_stride, int ntables,
                                   const uint16_t *d_quanta_out, int16_t *const d_coef_out[], const size_t out_stride[]);
/* single image, host tables (h_quanta_out NULL = h_quanta); synchronises */
int jpeg_amd_spectral_reduce(jpeg_amd_ctx *ctx, const jpeg_amd_layout *in_layout, int denom,
                             const int16_t *const d_coef_in[], const uint16_t *h_quanta, int ntables,
                             const uint16_t *h_quanta_out, int16_t *const d_coef_out[]);
/* File to file, built like jpeg_amd_transform: entropy decoding on the host (restart intervals on `nthreads` threads, <= 0:
 * all cores), ONE reduce launch on the GPU, and the host writer keeping the input's process, component ids, scan script,
 * table keys, restart interval and metadata segments verbatim and in order.  Every component of the frame is reduced.
 * h_requant: NULL (the file's own tables) or [ncomponents][64], the output tables (components that share a key must get
 * equal tables, else EINVAL).  h_out == NULL only sizes the output (*nbytes_out); out_info (optional) receives the output
 * frame. */
int jpeg_amd_reduce(jpeg_amd_ctx *ctx, const uint8_t *h_jpeg, size_t nbytes, int denom, const uint16_t *h_requant,
                    int nthreads, uint8_t *h_out, size_t capacity, size_t *nbytes_out, jpeg_amd_frame_info *out_info);

/* ---- files to tensors: JPEG files of mixed sizes and layouts to one training tensor in one call ------------------------
 * The file front end of the mixed calls: what a data loader has is a list of FILES -- a size per file, 4:2:0 beside 4:4:4,
 * some grey, some progressive -- and what it wants is one normalised [n, 3, Ht, Wt] tensor.
 *
 * 1. THE WINDOWED EXPAND.  jpeg_amd_spectral_expand_batch for images of different geometries in ONE launch, each plane cut
 * to a window of blocks and each block to its head.  Item i describes one image: its layout (units_x is the pitch of its
 * planes, in blocks), its planes d_coef[p] (device, whole planes of units_x * units_y blocks of 64 int16), per plane a window
 * (x, y, width, height in BLOCKS of that plane; width or height 0: nothing of the plane), `head`, the number of leading
 * 16-byte octets (eight coefficients in zigzag order) of each block to write, and where its sparse record lies in d_records:
 * its descriptors (one per block of the frame, as jpeg_amd_jpeg_decode_sparse orders them) at element desc_at and its
 * entries at element entries_at; a descriptor counts from entries_at.  The heads the view decode reads:
 *   denominator 8 reads zigzag index 0, denominator 4 indices 0 .. 4: both inside octet 0           head 1
 *   denominator 2 reads indices 0 .. 24: octets 0 .. 3                                              head 4
 *   denominator 1 reads the block                                                                   head 8
 * THE CONTRACT (the one statement of it): the bytes the call writes -- the first 16 * head bytes of every block of every
 * window -- are exactly the bytes jpeg_amd_spectral_expand_batch writes at the same addresses for the same record; every other
 * byte of the planes is left as it was, and is not read.  A descriptor of 0xFFFFFFFF gives zeros.  The entries of a block must
 * be in ascending zigzag order, as jpeg_amd_jpeg_decode_sparse and the encoders' sparse download write them: the walk of a
 * block stops at the first entry at or behind 8 * head.
 * h_items is a HOST array of n_images items; the call copies it before it returns.  Everything is judged before anything is
 * enqueued, the context last: EINVAL for n_images < 0 or above 65 535, null h_items or d_records, a layout
 * jpeg_amd_spectral_expand_batch refuses or whose blocks 32-bit descriptors cannot number, a head not in {1, 4, 8}, a plane
 * pointer that is null or not 16-byte aligned, a window outside its plane (or of negative width or height), and work
 * that does not fit a grid (2^31 - 1 workgroups of 256 octets); after a refused call nothing has been written.
 * n_images == 0 is OK.  Asynchronous on the context's stream.
 * Cost: one host-to-device copy of the item records, one launch; a work-item per octet written. */
typedef struct jpeg_amd_expand_item {
    jpeg_amd_layout layout;
    int16_t        *d_coef[JPEG_AMD_MAX_PLANES];
    jpeg_amd_region window[JPEG_AMD_MAX_PLANES];   /* blocks */
    int32_t         head;                          /* 1 | 4 | 8 octets */
    uint64_t        desc_at, entries_at;           /* elements into d_records */
} jpeg_amd_expand_item;
int jpeg_amd_spectral_expand_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_expand_item *h_items,
                                   const uint32_t *d_records);

/* 2. FILES TO A TENSOR, AND FILES TO RESIZED BYTES.  THE CONTRACT, by reference only -- no arithmetic is defined here: image i
 * of the output is, bit for bit, what jpeg_amd_decode_tensor_filter_mixed (jpeg_amd_decode_resized_filter_mixed for the byte
 * call) writes for file i when
 *   - the file is decoded by jpeg_amd_jpeg_decode_spectral into WHOLE planes, with the layout of its frame (component c's
 *     table is table c, ntables = its number of components), and
 *   - the view is the one the data-loader call chooses: denom = jpeg_amd_view_denom(source width, source height, out_w,
 *     out_h), region = jpeg_amd_view_of_source(that file's own size, denom, source rectangle),
 * with the same cosited, color, out_w, out_h, filter, spec and h_flip[i].  h_source_regions: a HOST array of n_images
 * rectangles in pixels of each file's full-size image, or NULL: the whole images.  h_info and h_views (optional, n_images
 * each) receive every file's frame and the view chosen for it; they are written as far as the files were judged, also by a
 * call that is then refused.  Output placement, strides, spec and h_flip as in the mixed calls.
 *
 * Everything that can be judged from the files' HEADERS is judged before anything is enqueued, the context last, file by file
 * in index order: a null file pointer (EINVAL), what jpeg_amd_jpeg_inspect says of the file, a frame that is not 8-bit with 1
 * or 3 components (ENOSUP: one such file refuses the whole call), a source rectangle outside the image (EINVAL); then, of
 * the files in front of the first offending one, whatever the mixed call refuses, the target included; last the antialias
 * filter's 16x limit or the bicubic filter's 8x limit (ENOSUP).  After a refused call nothing has been written and the context is usable.  n_images == 0 is OK.
 * A file whose entropy-coded data proves damaged AFTER the call has started ends the call with that file's status: every
 * copy and kernel in flight is waited for and the context stays usable, but output images of chunks already submitted MAY
 * HAVE BEEN WRITTEN.  There are no per-file statuses, and a bad file is not skipped.
 *
 * Route and cost.  The files go in CHUNKS of consecutive files, at most 32 and at most 1 GiB of coefficient planes (a larger
 * single file is a chunk of its own).  `nthreads` host threads (<= 0: all cores) beside the calling one entropy-decode the
 * files of ONE queue for the whole call, each into the SPARSE form (jpeg_amd_jpeg_decode_sparse), packed into a pinned slot
 * of the context; a file the sparse decoder does not take (progressive, a missing restart marker, too dense) is decoded into
 * planes there.  Per chunk ONE copy carries the tables, the item records and the packed records; planes of the dense files
 * go up whole; ONE launch of the windowed expand writes, for every sparse file, only the heads of the blocks of its view's
 * windows (jpeg_amd_view_window) into the context's plane buffer; then the mixed call runs on the chunk, as it stands.  Two
 * pinned slots: the threads decode chunk k + 1 while the device works on chunk k.  An image the tile kernels do not take
 * (cosited calls, factors 3 or 4, chroma not at 1x or 2x) is expanded whole, as its one-image fallback reads it whole.
 * A 224 x 224 crop of a 2000 x 1500 file at denominator 4 has 16 of 128 bytes written for the blocks under the crop and
 * nothing for the others; at denominator 1 the expand writes as much as jpeg_amd_spectral_expand_batch inside the window.
 * What is NOT saved: the entropy decoding of the whole file, and the planes keep their full pitch in device memory (the
 * plane buffer of the largest chunk stays in the context, as do two pinned slots of up to 1.8 times that).
 * Returns when the last chunk's kernels have finished. */
int jpeg_amd_decompress_tensor_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images,
                                     int nthreads, int cosited, jpeg_amd_color color,
                                     const jpeg_amd_region *h_source_regions, int32_t out_w, int32_t out_h, int filter,
                                     const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst, size_t dst_stride,
                                     jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views);
int jpeg_amd_decompress_resized_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[], int n_images,
                                      int nthreads, int cosited, jpeg_amd_color color,
                                      const jpeg_amd_region *h_source_regions, int32_t out_w, int32_t out_h, int filter,
                                      uint8_t *d_pixels, size_t pixel_stride, jpeg_amd_frame_info *h_info,
                                      jpeg_amd_view *h_views);

/* ---- oriented resample: the eight EXIF orientations in the resample stage of the tensor and file calls ------------------
 * A portrait photograph from a phone is STORED landscape, with Orientation = 6 in its EXIF segment; PIL's
 * ImageOps.exif_transpose, torchvision's decode_jpeg(apply_exif_orientation=True) and nvJPEG/DALI hand the loader the
 * upright image.  These calls do, in the resample stage: the oriented image is the stored one read with signed pixel and row
 * steps, so an orientation costs no pass of its own.  They also give callers flips, 90-degree rotations and transposes as a
 * per-image augmentation, with no EXIF involved.
 *
 * THE ORIENTATION.  A value o in 1 .. 8 is three bits (T, fx, fy):
 *     o          1      2      3      4      5      6      7      8
 *     T fx fy    0 0 0  0 1 0  0 1 1  0 0 1  1 0 0  1 0 1  1 1 1  1 1 0
 * For a stored image S of w x h the oriented image D is w' x h' = (T ? h : w) x (T ? w : h), and D[y'][x'] = S[ys][xs] with
 *     without T:  xs = fx ? w - 1 - x' : x',  ys = fy ? h - 1 - y' : y'
 *     with T:     xs = fx ? w - 1 - y' : y',  ys = fy ? h - 1 - x' : x'
 * (numpy: S[::-1] if fy, then [:, ::-1] if fx, then .transpose(1, 0, 2) if T; what PIL.ImageOps.exif_transpose gives.)
 * A rectangle (x', y', w_r', h_r') of D holds the pixels of the stored rectangle that jpeg_amd_orient_region gives: the
 * pairs swapped if T, then x = fx ? w - x_a - w_a : x_a, then y = fy ? h - y_a - h_a : y_a.
 *
 * THE CONTRACT, by reference only -- no arithmetic is defined here: an oriented resample of image i is the contract of its
 * filter ("resized decode" for JPEG_AMD_FILTER_BILINEAR, "antialiased resample" for JPEG_AMD_FILTER_ANTIALIAS, "bicubic
 * resample" for JPEG_AMD_FILTER_BICUBIC) applied to
 * the ORIENTED image, with w', h' in the place of w, h everywhere -- in kx = (float)w' / (float)out_w, in the clamps, and in
 * the tap limit, which is judged on the oriented factors; the horizontal pass runs along oriented x.  The output is, bit for
 * bit, what the call without orientations writes for a contiguous copy of the oriented pixels.  "tensor output" applies
 * behind it unchanged: h_flip mirrors the output along x, AFTER the orientation.
 *
 * THE CALLS.  Each takes the arguments of the *_filter_* call (or file call) it is named after, and h_orient, a HOST array of
 * n_images bytes, in front of the output pointer.  h_orient == NULL is, bit for bit and status for status, that call, and so
 * is an array of ones (it launches the same kernels from the same records); otherwise ONE launch of the oriented kernels
 * takes all the call's images, orientation 1 included.
 *   jpeg_amd_resize_oriented_batch, jpeg_amd_resize_oriented_tensor_batch: pixel sources, oriented whole.
 *   jpeg_amd_decode_resized_oriented_mixed, jpeg_amd_decode_tensor_oriented_mixed: the views stay in STORED scaled
 *     coordinates, as in the mixed calls; the orientation applies to each view's pixels.
 *   In these four a value outside 1 .. 8 is EINVAL, judged with image i's other arguments and behind them: in the resize
 *   calls behind the target and image i's extent, in the mixed calls behind image i's view and, for image 0, in front of
 *   the target.  The tap limit stays last.
 *   jpeg_amd_decompress_resized_oriented_mixed, jpeg_amd_decompress_tensor_oriented_mixed: the file calls.  Here
 *     h_orient[i] == JPEG_AMD_ORIENT_EXIF (0) means what jpeg_amd_jpeg_orientation says of file i, 1 .. 8 force a value, and
 *     a value above 8 is EINVAL, judged behind what the file call judges of file i's headers and in front of its rectangle.
 *     h_source_regions[i] is a rectangle of the ORIENTED full-size image -- the image the user sees -- or the whole of it
 *     (NULL); one outside the oriented image is EINVAL, where the file call judges its rectangle.  The denominator is
 *     jpeg_amd_view_denom(oriented rectangle's width, height, out_w, out_h), the view jpeg_amd_view_of_source of the STORED
 *     rectangle (jpeg_amd_orient_region), and h_views reports that stored view.  h_orient_out (optional, n_images values)
 *     receives the orientation applied to each file, written as far as the files were judged.  Contract by reference, as in
 *     "files to tensors": image i is what jpeg_amd_decode_tensor_oriented_mixed (jpeg_amd_decode_resized_oriented_mixed)
 *     writes for the file decoded whole, with that view and that orientation.
 * There are no oriented forms of the uniform *_batch decodes (the mixed calls serve them), of the region, scaled and view
 * byte calls, of the full decode or of the encoders.  Nothing is oriented in the coefficient domain: the lossless transforms
 * cannot orient an image whose size is no multiple of its MCU.
 * Cost: the route of the call it is named after.  With a transposing orientation (5 .. 8) neighbouring work-items read
 * bytes one stored row apart instead of 3 bytes apart: more cache lines per load, the same lines per tile. */
enum {
    JPEG_AMD_ORIENT_EXIF = 0,    /* the file calls only: the file's own tag */
    JPEG_AMD_ORIENT_1 = 1,       /* as stored */
    JPEG_AMD_ORIENT_2 = 2,       /* mirrored along x */
    JPEG_AMD_ORIENT_3 = 3,       /* rotated by 180 degrees */
    JPEG_AMD_ORIENT_4 = 4,       /* mirrored along y */
    JPEG_AMD_ORIENT_5 = 5,       /* transposed */
    JPEG_AMD_ORIENT_6 = 6,       /* rotated by 90 degrees clockwise */
    JPEG_AMD_ORIENT_7 = 7,       /* transposed along the other diagonal */
    JPEG_AMD_ORIENT_8 = 8        /* rotated by 90 degrees counter-clockwise */
};

/* JPEG.EXIF.parse and its subscript(tag:) (metadata.swift:440-560), for the Orientation field (tag 0x0112) alone: a marker
 * walk from SOI to the first SOS; of the first APP1 whose payload begins "Exif\0\0" the TIFF header ("II*\0" or "MM\0*") and
 * the offset of IFD0; of IFD0's 12-byte entries the first with tag 0x0112, type SHORT (3) or LONG (4) and count 1, whose
 * value is read in the file's byte order from the start of the value field.  EINVAL for null pointers; OK in every other
 * case, with *orientation = 1 unless a value in 1 .. 8 was found: no EXIF or no tag, a value outside 1 .. 8, another type or
 * count, an offset or an entry count that leaves the segment, a segment length that leaves the file, and input that is no
 * JPEG at all give 1.  Whether the file is decodable is jpeg_amd_jpeg_inspect's verdict: a broken EXIF block never fails a
 * decode.  No byte at or beyond nbytes is read; only IFD0 is looked at.  Host only.
 * (jpeg_amd_transform keeps APPn segments verbatim, this tag included: it does not reset it.) */
int jpeg_amd_jpeg_orientation(const uint8_t *h_jpeg, size_t nbytes, int32_t *orientation);
/* THE ORIENTATION's rectangle mapping for a stored frame of width x height: `oriented`, a rectangle of the oriented image
 * (NULL: the whole of it), as the stored rectangle that holds its pixels.  EINVAL for an orientation outside 1 .. 8, a
 * width or height below 1, a null `stored`, and a rectangle that is empty or not inside the oriented image.  Host only, pure. */
int jpeg_amd_orient_region(int orientation, int32_t width, int32_t height, const jpeg_amd_region *oriented,
                           jpeg_amd_region *stored);

int jpeg_amd_resize_oriented_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                   const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, int filter,
                                   const uint8_t *h_orient, uint8_t *d_dst, size_t dst_stride);
int jpeg_amd_resize_oriented_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                          const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, int filter,
                                          const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, const uint8_t *h_orient,
                                          void *d_dst, size_t dst_stride);
int jpeg_amd_decode_resized_oriented_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                           jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                           int filter, const uint8_t *h_orient, uint8_t *d_pixels, size_t pixel_stride);
int jpeg_amd_decode_tensor_oriented_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                          jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                          int filter, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                          const uint8_t *h_orient, void *d_dst, size_t dst_stride);
int jpeg_amd_decompress_tensor_oriented_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                                              int n_images, int nthreads, int cosited, jpeg_amd_color color,
                                              const jpeg_amd_region *h_source_regions, int32_t out_w, int32_t out_h,
                                              int filter, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                              const uint8_t *h_orient, void *d_dst, size_t dst_stride,
                                              jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views, int32_t *h_orient_out);
int jpeg_amd_decompress_resized_oriented_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                                               int n_images, int nthreads, int cosited, jpeg_amd_color color,
                                               const jpeg_amd_region *h_source_regions, int32_t out_w, int32_t out_h,
                                               int filter, const uint8_t *h_orient, uint8_t *d_pixels, size_t pixel_stride,
                                               jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views, int32_t *h_orient_out);

/* ---- placed resample: the image in a window of the output canvas, a constant fill around it (letterbox) ------------------
 *
 * Every resample call stretches its source over the whole out_w x out_h target.  These calls keep the target as a CANVAS and
 * resample image i into a WINDOW (x0, y0, ww, wh) of it -- jpeg_amd_region's x, y, width, height -- and write the call's
 * FILL, three bytes, everywhere else: the letterbox of a detector, "pad to square", fill_values.  One launch still writes every
 * image of the call, whatever their windows.
 *
 * THE CONTRACT, by reference only -- no arithmetic is defined here.  Canvas pixel (X, Y) is the pixel STORED at column
 * flip ? out_w - 1 - X : X of row Y: the flip of "tensor output" mirrors the whole canvas, window position included, behind
 * everything else.
 *   Inside the window, x0 <= X < x0 + ww and y0 <= Y < y0 + wh, canvas pixel (X, Y) is, bit for bit, output pixel
 *     (X - x0, Y - y0) of the filter's contract ("resized decode", "antialiased resample", "bicubic resample") for a target of
 *     ww x wh, applied to the oriented image where the call names an orientation ("oriented resample").  ww, wh stand in the
 *     place of out_w, out_h everywhere in that contract: in kx = (float)w' / (float)ww, in sx and rx, and in the tap limit --
 *     16 (bicubic: 8) is judged on the window's factors, never the canvas's.
 *   Outside the window the byte of channel c is fill[c].
 *   "tensor output" applies behind this unchanged: a padded element is what that contract gives for the byte fill[c],
 *     ((float)fill[c] - mean[c]) * scale[c] converted; a fill equal to the rounded mean gives about 0.
 *   In the view and file calls the denominator is jpeg_amd_view_denom(source rectangle's (oriented) width, height, ww, wh):
 *     chosen against the window, never the canvas.
 *
 * THE WINDOWS.  mode JPEG_AMD_PLACE_WINDOWS: the caller's, h_windows[i] for image i.  JPEG_AMD_PLACE_FIT: the largest window
 * of the source's aspect ratio that the canvas holds; JPEG_AMD_PLACE_FIT_DOWN: the source's own size where the canvas holds it
 * (nothing is enlarged), FIT otherwise; both at `anchor`.  jpeg_amd_place_window states the integers; the source size it
 * takes is the ORIENTED image's (the resize calls), the oriented view rectangle's (the mixed calls) or the oriented source
 * rectangle's of the full-size image (the file calls).
 *
 * THE CALLS.  Each takes the arguments of the *_oriented_* call it is named after (h_orient NULL allowed, as there) and, in
 * front of the output pointer, `place` and h_windows_out: n_images entries that receive the window applied to each image, or
 * NULL; the file calls write it as far as the files were judged, like h_views.  place == NULL is, bit for bit and status for
 * status, the oriented call: the same records, the same kernels.  A placed call writes placed records for all its images and
 * ONE launch of the placed kernels takes them (orientation 1: steps 3 and 3 w).  EINVAL, judged with the target (mode,
 * anchor, missing windows) and per image behind its orientation (the window), the tap limit staying last: an unknown mode or
 * anchor; mode WINDOWS with h_windows NULL and n_images > 0; a window with ww < 1 or wh < 1; a window not inside the canvas.
 * Nothing is enqueued, and the device is not touched, for a call that is refused.
 *
 * There are no placed forms of the uniform *_batch decodes (the mixed calls serve them), of the region, scaled and view byte
 * calls or of the encoders; no per-image output size, no border mode but the constant, no fill per image. */
enum {
    JPEG_AMD_PLACE_WINDOWS = 0,   /* h_windows given */
    JPEG_AMD_PLACE_FIT = 1,       /* aspect-preserving, one side of the window equals the canvas's */
    JPEG_AMD_PLACE_FIT_DOWN = 2   /* FIT, but never enlarging */
};
enum {
    JPEG_AMD_ANCHOR_CENTRE = 0,
    JPEG_AMD_ANCHOR_TOP_LEFT = 1
};
typedef struct {
    int32_t mode;                       /* JPEG_AMD_PLACE_* */
    int32_t anchor;                     /* JPEG_AMD_ANCHOR_*; positions the window in the FIT modes */
    const jpeg_amd_region *h_windows;   /* n_images, mode WINDOWS only */
    uint8_t fill[3];
    uint8_t reserved;
} jpeg_amd_placement;

/* The window of the FIT modes for a source of src_w x src_h on a canvas of out_w x out_h, in integers.
 *   FIT: if (int64)out_w * src_h <= (int64)out_h * src_w the width binds: ww = out_w and
 *     wh = min(out_h, max(1, (2 * src_h * out_w + src_w) / (2 * src_w))) (the quotient rounded to nearest, in int64);
 *     otherwise the same with the roles of the two axes swapped.
 *   FIT_DOWN: ww = src_w, wh = src_h if src_w <= out_w and src_h <= out_h; FIT otherwise.
 *   CENTRE: x0 = (out_w - ww) / 2, y0 = (out_h - wh) / 2.  TOP_LEFT: x0 = y0 = 0.
 * EINVAL: a mode other than FIT and FIT_DOWN, an unknown anchor, a size below 1, a canvas side above 2^30, a null `window`.
 * Host only, pure. */
int jpeg_amd_place_window(int mode, int anchor, int32_t src_w, int32_t src_h, int32_t out_w, int32_t out_h,
                          jpeg_amd_region *window);

int jpeg_amd_resize_placed_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                 const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, int filter,
                                 const uint8_t *h_orient, const jpeg_amd_placement *place, jpeg_amd_region *h_windows_out,
                                 uint8_t *d_dst, size_t dst_stride);
int jpeg_amd_resize_placed_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                        const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, int filter,
                                        const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, const uint8_t *h_orient,
                                        const jpeg_amd_placement *place, jpeg_amd_region *h_windows_out, void *d_dst,
                                        size_t dst_stride);
int jpeg_amd_decode_resized_placed_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                         jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                         int filter, const uint8_t *h_orient, const jpeg_amd_placement *place,
                                         jpeg_amd_region *h_windows_out, uint8_t *d_pixels, size_t pixel_stride);
int jpeg_amd_decode_tensor_placed_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                        jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                        int filter, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                        const uint8_t *h_orient, const jpeg_amd_placement *place,
                                        jpeg_amd_region *h_windows_out, void *d_dst, size_t dst_stride);
int jpeg_amd_decompress_tensor_placed_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                                            int n_images, int nthreads, int cosited, jpeg_amd_color color,
                                            const jpeg_amd_region *h_source_regions, int32_t out_w, int32_t out_h,
                                            int filter, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                            const uint8_t *h_orient, const jpeg_amd_placement *place,
                                            jpeg_amd_region *h_windows_out, void *d_dst, size_t dst_stride,
                                            jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views, int32_t *h_orient_out);
int jpeg_amd_decompress_resized_placed_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                                             int n_images, int nthreads, int cosited, jpeg_amd_color color,
                                             const jpeg_amd_region *h_source_regions, int32_t out_w, int32_t out_h,
                                             int filter, const uint8_t *h_orient, const jpeg_amd_placement *place,
                                             jpeg_amd_region *h_windows_out, uint8_t *d_pixels, size_t pixel_stride,
                                             jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views, int32_t *h_orient_out);

/* ---- warped resample: rotate, shear and scale through an affine map, in the resample launch -----------------------------
 *
 * Every call above resamples along the axes.  These calls take, per image, a matrix m[6] = (m00, m01, m02, m10, m11, m12) of
 * binary32 that maps the centre of an OUTPUT pixel to a point of the SOURCE, both in continuous pixel coordinates: pixel i
 * covers [i, i + 1) and its centre is i + 0.5.  It is the INVERSE map, the one grid_sample and torchvision's affine use:
 * RandomRotation, RandomAffine, the rotation, shear and scale of a detector's augmentation, deskewing a scan.  One launch
 * writes every image of the call.
 *
 * THE CONTRACT.  A source of w x h pixels of 3 bytes, a target of out_w x out_h.  Every statement is ONE binary32 operation
 * and nothing is contracted.  For stored output column x and row y:
 *     xs = flip ? out_w - 1 - x : x             (tensor calls: the WARPED image mirrored, as "tensor output" says; else x)
 *     xc = (float)xs + 0.5f;   yc = (float)y + 0.5f
 *     sx = ((m00 * xc) + (m01 * yc)) + m02;   sx = sx - 0.5f;   sx = min(max(sx, -1.0f), (float)w)
 *     sy = ((m10 * xc) + (m11 * yc)) + m12;   sy = sy - 0.5f;   sy = min(max(sy, -1.0f), (float)h)
 *     fx0 = floorf(sx);  x0 = (int)fx0;  x1 = x0 + 1;  fx = sx - fx0          (x0 in -1 .. w)
 *     fy0 = floorf(sy);  y0 = (int)fy0;  y1 = y0 + 1;  fy = sy - fy0          (y0 in -1 .. h)
 *     a, b, c, d = the taps (y0, x0), (y0, x1), (y1, x0), (y1, x1) of the channel, as float
 *     top = a + fx * (b - a);  bot = c + fx * (d - c);  v = top + fy * (bot - top)
 *     out = (uint8)(int)(min(max(v, 0.0f), 255.0f) + 0.5f)
 * The last two lines are those of "resized decode".  A tap whose column is outside 0 .. w - 1 or whose row is outside
 * 0 .. h - 1 has, by the call's edge mode,
 *   JPEG_AMD_EDGE_FILL (0): the value (float)fill[c] -- grid_sample's "zeros" padding with torchvision's fill.  The image's
 *     border blends into the fill over one pixel, and a pixel well outside the source is the fill exactly (a = b = c = d
 *     gives v = a);
 *   JPEG_AMD_EDGE_REPLICATE (1): its indices clamped into the image -- grid_sample's "border".
 * The filter is the two-tap one at any reduction: there is no tap limit and no ENOSUP.  The tensor output is "tensor output"
 * applied to this byte, fill pixels included.
 *
 * CONSEQUENCES.  The identity (1, 0, 0, 0, 1, 0) at out = (w, h) gives the source bytes.  A translation by integers gives the
 * bytes shifted, and the fill (or the replicated edge) where they came from outside.  (w / out_w, 0, 0, 0, h / out_h, 0),
 * divided in binary32, with REPLICATE is jpeg_amd_resize_batch's output bit for bit.  (0, 1, 0, -1, 0, h) to out = (h, w) is
 * the image rotated by 90 degrees clockwise, as a permutation of bytes.  Against grid_sample(bilinear, align_corners=False)
 * with "zeros" and "border" the bytes agree within one level (the order of the operations differs).
 *
 * EINVAL: a matrix entry that is not finite or exceeds 2^30 in magnitude (with an output side of at most 2^30 no coordinate
 * overflows and no NaN arises); a source side above 2^24 ((float)w must be exact); an edge mode other than 0 and 1; a null
 * h_matrices with n_images > 0, a null `warp`; and whatever jpeg_amd_resize_batch or jpeg_amd_tensor_extent refuse.
 * Everything is judged before anything is enqueued, the context last; n_images == 0 is OK. */
enum {
    JPEG_AMD_EDGE_FILL = 0,
    JPEG_AMD_EDGE_REPLICATE = 1
};
typedef struct {
    int32_t edge;       /* JPEG_AMD_EDGE_* */
    uint8_t fill[3];    /* EDGE_FILL: the bytes of a tap outside the image */
} jpeg_amd_warp;

/* Pixels to pixels, one launch: jpeg_amd_resize_batch's and jpeg_amd_resize_tensor_batch's arguments, and h_matrices
 * ([n_images][6], host, copied before the call returns) and `warp` behind the extents. */
int jpeg_amd_warp_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                        const jpeg_amd_extent *h_extents, const float *h_matrices, const jpeg_amd_warp *warp,
                        int32_t out_w, int32_t out_h, uint8_t *d_dst, size_t dst_stride);
int jpeg_amd_warp_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                               const jpeg_amd_extent *h_extents, const float *h_matrices, const jpeg_amd_warp *warp,
                               int32_t out_w, int32_t out_h, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                               void *d_dst, size_t dst_stride);

/* The view of an image that a warp reads, and the matrix against that view.  Host only, pure, computed in double.
 * `m` is in the coordinates of the UPRIGHT image: the stored W x H image of `layout` seen through `orientation` 1 .. 8
 * ("oriented resample").
 *   1. The orientation is composed into the matrix.  With the orientation's bits (T, fx, fy) and (Xu, Yu) = m applied to an
 *      output centre: (a, b) = T ? (Yu, Xu) : (Xu, Yu), Xs = fx ? W - a : a, Ys = fy ? H - b : b.  The result M_s maps output
 *      centres to STORED coordinates; its linear part is m's entries permuted and negated, which is exact.
 *   2. The denominator: the largest d in {8, 4, 2, 1} with d * d <= min(m00 m00 + m10 m10, m01 m01 + m11 m11).  Both output
 *      axes then step at least d source pixels, so the image at 1/d still needs no enlarging: jpeg_amd_view_denom's rule for
 *      a map without a rectangle.
 *   3. M_s times 1/d (exact): the matrix against the scaled image of W' x H' (jpeg_amd_scaled_layout).
 *   4. The footprint: the canvas corners (0, 0), (out_w, 0), (0, out_h), (out_w, out_h) through it, X = (s00 cx + s01 cy)
 *      + s02; with xmin, xmax the extremes the view's columns are clamp(floor(xmin - 0.5) - 1, 0, W' - 1) ..=
 *      clamp(floor(xmax - 0.5) + 2, 0, W' - 1), its rows likewise.  The margin of one pixel beyond the taps covers the
 *      binary32 rounding of the kernel's coordinates.  The view is never empty; where its edge lies inside the image no tap
 *      reaches it, and where its edge is the image's, fill and replication mean there what they mean for the whole image.
 *   5. m_view: that matrix with the view's x and y subtracted from its m02 and m12, rounded to binary32 ONCE.
 * EINVAL: an orientation outside 1 .. 8, a matrix the contract refuses, out_w or out_h outside 1 .. 2^30, a layout
 * jpeg_amd_scaled_layout refuses, a null pointer. */
int jpeg_amd_warp_view(const jpeg_amd_layout *layout, int orientation, const float m[6], int32_t out_w, int32_t out_h,
                       jpeg_amd_view *view, float m_view[6]);

/* The decode and file routes, by reference only: they define no arithmetic.
 * jpeg_amd_decode_warped_mixed / jpeg_amd_decode_tensor_warped_mixed: jpeg_amd_decode_resized_mixed's and
 * jpeg_amd_decode_tensor_mixed's arguments without h_views; h_orient (n_images values in 1 .. 8, NULL = all 1), h_matrices
 * (upright coordinates of the FULL-SIZE images) and `warp`; h_views_out and h_matrices_out ([n_images] and [n_images][6], or
 * NULL) receive what jpeg_amd_warp_view gave.  Image i is, bit for bit, jpeg_amd_warp_batch (or the tensor form) applied to
 * the pixels jpeg_amd_decode_view_batch defines for the view jpeg_amd_warp_view returns, with the m_view it returns.  The
 * route is the resized calls': the mixed view decode per chunk, then ONE warp launch per chunk.
 * jpeg_amd_decompress_resized_warped_mixed / jpeg_amd_decompress_tensor_warped_mixed: their file front end, as "files to
 * tensors" is of the mixed calls: h_orient as in the *_oriented_mixed file calls (JPEG_AMD_ORIENT_EXIF = the file's own tag),
 * each file's view from jpeg_amd_warp_view; h_info, h_views, h_matrices_out and h_orient_out are written as far as the files
 * were judged.  There are no source rectangles (the matrix says what is read), no placement and no filter but the bilinear
 * (the projective calls have the bicubic one: "bicubic warp"). */
int jpeg_amd_decode_warped_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                 jpeg_amd_color color, const uint8_t *h_orient, const float *h_matrices,
                                 const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h, jpeg_amd_view *h_views_out,
                                 float *h_matrices_out, uint8_t *d_pixels, size_t pixel_stride);
int jpeg_amd_decode_tensor_warped_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                        jpeg_amd_color color, const uint8_t *h_orient, const float *h_matrices,
                                        const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h,
                                        const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, jpeg_amd_view *h_views_out,
                                        float *h_matrices_out, void *d_dst, size_t dst_stride);
int jpeg_amd_decompress_resized_warped_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                                             int n_images, int nthreads, int cosited, jpeg_amd_color color,
                                             const uint8_t *h_orient, const float *h_matrices, const jpeg_amd_warp *warp,
                                             int32_t out_w, int32_t out_h, uint8_t *d_pixels, size_t pixel_stride,
                                             jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views, float *h_matrices_out,
                                             int32_t *h_orient_out);
int jpeg_amd_decompress_tensor_warped_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                                            int n_images, int nthreads, int cosited, jpeg_amd_color color,
                                            const uint8_t *h_orient, const float *h_matrices, const jpeg_amd_warp *warp,
                                            int32_t out_w, int32_t out_h, const jpeg_amd_tensor_spec *spec,
                                            const uint8_t *h_flip, void *d_dst, size_t dst_stride,
                                            jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views, float *h_matrices_out,
                                            int32_t *h_orient_out);

/* ---- colour stage: an affine map of (R, G, B) per image between the resample and the tensor output -------------------------
 *
 * Brightness, contrast, saturation and hue jitter, a drop to grey, BGR order, a single luma value: each is one affine map of
 * a pixel's (R, G, B) -- a 3 x 3 matrix and an offset -- followed by a clamp, and so is any composition of them.  The calls
 * below apply one such map per image inside the resample launch of the tensor calls, between the byte the resample defines
 * and the (u - mean) * scale of "tensor output".
 *
 * THE CONTRACT.  The colour stage defines no resample arithmetic.  Let u(i, y, xs, c) be the byte the underlying call -- the
 * placed resample with any of the three filters, or the warped resample -- defines for image i at stored column x, after the
 * flip (xs = flip ? out_w - 1 - x : x); fill pixels of a placement or a warp count as pixels.  With
 * r, g, b = (float)u(.., 0), (float)u(.., 1), (float)u(.., 2) and image i's twelve binary32 numbers k[c][0 .. 3], for every
 * channel c, every statement ONE binary32 operation and nothing contracted:
 *     p = ((k[c][0] * r) + (k[c][1] * g)) + (k[c][2] * b)
 *     q = p + k[c][3]
 *     q = q < lo ? lo : q;   q = q > hi ? hi : q        (lo, hi per call, in byte units)
 *     t = q - mean[c];  v = t * scale[c];  element = v converted                  ("tensor output", unchanged)
 * The clamp is two comparisons and selects, so that it is defined for zeros of either sign: -0 is not below +0 and stays.
 * lo = -infinity and hi = +infinity clamp nothing: q is finite.
 *
 * CONSEQUENCES.  The identity matrix with offset 0 and no clamp is the underlying tensor call bit for bit (1 * r, + 0 * g,
 * + 0 * b and + 0 are exact for r, g, b >= 0, and give +0 for 0).  A permutation matrix is that call with the channels
 * permuted, bit for bit (BGR).  Three equal rows give three equal q (greyscale).  The fill is transformed like any pixel.
 *
 * EINVAL, judged with the target, before anything is enqueued and with the context judged last: an entry that is not finite
 * or exceeds 2^30 in magnitude (so that no NaN or infinity can arise); lo or hi that is a NaN; lo > hi; a null h_matrices
 * with n_images > 0.  (The colour stage exists for the tensor calls only: the byte calls have no colour forms.) */
typedef struct {
    const float *h_matrices;   /* [n_images][12], host: image i's row c is k[c][0 .. 3]; copied before the call returns */
    float lo, hi;              /* the clamp, in byte units; -INFINITY and INFINITY: none */
} jpeg_amd_colour;

/* Each call takes the arguments of the call it is named after and `colour` in front of the output pointer: _resize_colour_
 * tensor_batch of jpeg_amd_resize_placed_tensor_batch, _decode_tensor_colour_mixed of jpeg_amd_decode_tensor_placed_mixed,
 * _decompress_tensor_colour_mixed of jpeg_amd_decompress_tensor_placed_mixed, _warp_colour_tensor_batch of
 * jpeg_amd_warp_tensor_batch, and the two *_warped_colour_mixed calls of the *_warped_mixed tensor calls.  With colour == NULL
 * each IS that call, status for status and bit for bit.  With a colour the route is that call's -- one resample launch per
 * call or chunk, the colour records in the same upload as the resample records -- and a call without a placement writes
 * placed records whose window is the whole canvas, which "placed resample" makes the oriented and the stored call. */
int jpeg_amd_resize_colour_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                        const jpeg_amd_extent *h_extents, int32_t out_w, int32_t out_h, int filter,
                                        const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, const uint8_t *h_orient,
                                        const jpeg_amd_placement *place, jpeg_amd_region *h_windows_out,
                                        const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride);
int jpeg_amd_decode_tensor_colour_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                        jpeg_amd_color color, const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h,
                                        int filter, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                        const uint8_t *h_orient, const jpeg_amd_placement *place,
                                        jpeg_amd_region *h_windows_out, const jpeg_amd_colour *colour, void *d_dst,
                                        size_t dst_stride);
int jpeg_amd_decompress_tensor_colour_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                                            int n_images, int nthreads, int cosited, jpeg_amd_color color,
                                            const jpeg_amd_region *h_source_regions, int32_t out_w, int32_t out_h,
                                            int filter, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                            const uint8_t *h_orient, const jpeg_amd_placement *place,
                                            jpeg_amd_region *h_windows_out, const jpeg_amd_colour *colour, void *d_dst,
                                            size_t dst_stride, jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views,
                                            int32_t *h_orient_out);
int jpeg_amd_warp_colour_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                      const jpeg_amd_extent *h_extents, const float *h_matrices, const jpeg_amd_warp *warp,
                                      int32_t out_w, int32_t out_h, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                      const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride);
int jpeg_amd_decode_tensor_warped_colour_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                               jpeg_amd_color color, const uint8_t *h_orient, const float *h_matrices,
                                               const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h,
                                               const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                               jpeg_amd_view *h_views_out, float *h_matrices_out,
                                               const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride);
int jpeg_amd_decompress_tensor_warped_colour_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                                                   int n_images, int nthreads, int cosited, jpeg_amd_color color,
                                                   const uint8_t *h_orient, const float *h_matrices,
                                                   const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h,
                                                   const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                                   const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride,
                                                   jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views,
                                                   float *h_matrices_out, int32_t *h_orient_out);

/* ---- projective resample: a 3 x 3 homography in the warp calls ---------------------------------------------------------------
 *
 * The warp calls take an affine map.  These take, per image, a matrix m[9] = (m00, m01, m02, m10, m11, m12, m20, m21, m22) of
 * binary32, row by row: the INVERSE projective map from the centre of an OUTPUT pixel to a point of the SOURCE, in the
 * continuous pixel coordinates of "warped resample".  It is torchvision's RandomPerspective and perspective(), the keystone
 * correction of a photographed page, sign or number plate, the bird's-eye view of a road camera.  One launch writes every
 * image of the call.
 *
 * THE CONTRACT.  A source of w x h pixels of 3 bytes, a target of out_w x out_h.  Every statement is ONE binary32 operation
 * and nothing is contracted; xs, xc, yc are those of "warped resample":
 *     nx = ((m00 * xc) + (m01 * yc)) + m02
 *     ny = ((m10 * xc) + (m11 * yc)) + m12
 *     nw = ((m20 * xc) + (m21 * yc)) + m22
 *     rw = 1.0f / nw                                      (the correctly rounded binary32 quotient)
 *     sx = nx * rw;   sx = sx - 0.5f;   sx = min(max(sx, -1.0f), (float)w)
 *     sy = ny * rw;   sy = sy - 0.5f;   sy = min(max(sy, -1.0f), (float)h)
 * and from fx0 = floorf(sx) on the contract is "warped resample" word for word: the four taps, JPEG_AMD_EDGE_FILL and
 * JPEG_AMD_EDGE_REPLICATE of the same jpeg_amd_warp, the blend, the rounding to a byte, "tensor output" and the "colour stage"
 * behind it.
 *
 * CONSEQUENCE.  With the last row (0, 0, 1): nw = (0 + 0) + 1 = 1, rw = 1 and sx = nx * 1 = nx exactly, so the call is
 * jpeg_amd_warp_batch on m[0 .. 5] (or its tensor and colour forms), bit for bit.
 *
 * THE LIMITS, derived.  The entries are finite and at most 2^30 in magnitude, as a warp's.  The denominator is the affine
 * form W(cx, cy) = m20 cx + m21 cy + m22 of the canvas point; with S = |m20| out_w + |m21| out_h + |m22|, |W| <= S on the
 * canvas, and W, being affine, takes its minimum over the canvas at one of the four corners (0, 0), (out_w, 0), (0, out_h),
 * (out_w, out_h).  A matrix is refused unless S >= 2^-30 and that minimum is at least S / 16.  Then at every pixel centre:
 *   - the exact W is at least S / 16, and the computed nw differs from it by at most about 3 * 2^-24 * S (two products and two
 *     sums, each rounded once, of terms that are at most S), that is by at most 3 * 2^-20 of W itself: nw is positive, at
 *     least 2^-35 and at most 3 * 2^60, normal in binary32, and so is rw; the division meets no zero, no subnormal and no
 *     infinity;
 *   - |nx| and |ny| are below 3 * 2^60, so |nx * rw| is below 2^97: every coordinate is finite, no NaN arises, and the clamp
 *     is defined;
 *   - the foreshortening across the canvas, max W / min W, is at most 16 : 1, far beyond the distortion_scale = 0.5 of the
 *     usual augmentation; the horizon W = 0 is never on the canvas.
 *
 * EINVAL, judged on the host in double before anything is enqueued, the context last: an entry that is not finite or exceeds
 * 2^30 in magnitude; S < 2^-30; min W < S / 16 (a corner with W <= 0 is such a matrix); and whatever "warped resample"
 * refuses otherwise.  n_images == 0 is OK.
 *
 * h_matrices is [n_images][9].  jpeg_amd_project_tensor_batch takes `colour` in front of the output pointer: NULL for none,
 * else the "colour stage" as jpeg_amd_warp_colour_tensor_batch applies it -- one entry point, not two. */
int jpeg_amd_project_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                           const jpeg_amd_extent *h_extents, const float *h_matrices, const jpeg_amd_warp *warp,
                           int32_t out_w, int32_t out_h, uint8_t *d_dst, size_t dst_stride);
int jpeg_amd_project_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                  const jpeg_amd_extent *h_extents, const float *h_matrices, const jpeg_amd_warp *warp,
                                  int32_t out_w, int32_t out_h, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                  const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride);

/* The view of an image that a projective map reads, and the matrix against that view: jpeg_amd_warp_view for a homography.
 * Host only, pure, computed in double.  `m` is in the coordinates of the UPRIGHT image, as there.
 *   1. The orientation is composed into the matrix, row by row (row k = (mk0, mk1, mk2); row 2 is the denominator's): with the
 *      orientation's bits (T, fx, fy), T swaps rows 0 and 1; fx: row0 = W row2 - row0; fy: row1 = H row2 - row1.  The result
 *      maps output centres to STORED coordinates, since W - nx / nw = (W nw - nx) / nw.
 *   2. The denominator.  The Jacobian of (X, Y) = (nx, ny) / nw has the columns ((m00 - X m20) / nw, (m10 - Y m20) / nw) and
 *      ((m01 - X m21) / nw, (m11 - Y m21) / nw): the source steps of one output column and of one output row.  They are taken
 *      at the four canvas corners and at the canvas centre (out_w / 2, out_h / 2), and d is the largest of {8, 4, 2, 1} with
 *      d * d <= the minimum of the ten squared column norms.  For a last row (0, 0, 1) this is jpeg_amd_warp_view's rule.  For
 *      a true projective map the five points are a RULE, not a bound: the step varies over the canvas and may be smaller
 *      between them.  Any d gives a result that the contract defines (image i is the project call on the view's pixels); d
 *      decides only the cost and the sharpness.
 *   3. Rows 0 and 1 times 1 / d (exact): the matrix against the scaled image of W' x H' (jpeg_amd_scaled_layout).
 *   4. The footprint.  nw > 0 on the canvas, so the canvas maps onto the convex quadrilateral of its corners' images, and the
 *      extremes xmin, xmax, ymin, ymax are those of the four corners, each divided in double.  The view's columns are
 *      clamp(floor(xmin - 0.5) - 1, 0, W' - 1) ..= clamp(floor(xmax - 0.5) + 2, 0, W' - 1), its rows likewise; it is never
 *      empty.  The margin of one pixel beyond the taps covers the binary32 rounding of the kernel's coordinate, which is
 *      bounded as follows.  Let X be the exact coordinate against the view and A = (|m00 xc| + |m01 yc| + |m02|) / nw the sum
 *      of the magnitudes of its three terms.  nx carries at most 3 * 2^-24 * A * nw (as nw's bound above), which is
 *      3 * 2^-24 * A of X; nw carries 3 * 2^-20 of itself, the quotient, the product and the subtraction of 0.5 one rounding
 *      each, together 51 * 2^-24 * |X|; and rounding m_view to binary32 adds at most 2^-24 * A from row 0 and 16 * 2^-24 * |X|
 *      from row 2.  In all |error| <= 2^-24 * (67 |X| + 4 A).  With |X| <= 2^16, the largest side a JPEG can have, and
 *      A <= 2^18 (terms that cancel from no more than four times that side: every rotation, shear and keystone about a point
 *      of the image), this is 67 * 2^-8 + 4 * 2^-6 < 0.33 pixel: the one-pixel margin holds for every source a JPEG file can
 *      hold, and is not widened.  A matrix whose terms cancel from further out loses bits in proportion, as an affine one
 *      does in "warped resample"; the call remains defined by the view and m_view it returns.
 *   5. m_view: row0 - x_view row2 and row1 - y_view row2, row 2 unchanged, rounded to binary32 ONCE.  It passes the contract's
 *      own check, or the call is refused (an entry beyond 2^30 behind the subtraction).
 * EINVAL: an orientation outside 1 .. 8, a matrix the contract refuses on this canvas, out_w or out_h outside 1 .. 2^30, a
 * layout jpeg_amd_scaled_layout refuses, a null pointer. */
int jpeg_amd_project_view(const jpeg_amd_layout *layout, int orientation, const float m[9], int32_t out_w, int32_t out_h,
                          jpeg_amd_view *view, float m_view[9]);

/* The decode and file routes, by reference only: they define no arithmetic.  Each is the *_warped_mixed call of the same
 * place with h_matrices and h_matrices_out of [n_images][9], jpeg_amd_project_view where that call has jpeg_amd_warp_view,
 * and ONE project launch per chunk: image i is, bit for bit, jpeg_amd_project_batch (or the tensor form) applied to the pixels
 * jpeg_amd_decode_view_batch defines for the view jpeg_amd_project_view returns, with the m_view it returns.  The tensor
 * forms take `colour` in front of the output pointer, NULL for none.  The file calls honour JPEG_AMD_ORIENT_EXIF, and write
 * h_info, h_views, h_matrices_out and h_orient_out as far as the files were judged. */
int jpeg_amd_decode_projected_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                    jpeg_amd_color color, const uint8_t *h_orient, const float *h_matrices,
                                    const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h, jpeg_amd_view *h_views_out,
                                    float *h_matrices_out, uint8_t *d_pixels, size_t pixel_stride);
int jpeg_amd_decode_tensor_projected_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                           jpeg_amd_color color, const uint8_t *h_orient, const float *h_matrices,
                                           const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h,
                                           const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                           jpeg_amd_view *h_views_out, float *h_matrices_out,
                                           const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride);
int jpeg_amd_decompress_resized_projected_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                                                int n_images, int nthreads, int cosited, jpeg_amd_color color,
                                                const uint8_t *h_orient, const float *h_matrices,
                                                const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h, uint8_t *d_pixels,
                                                size_t pixel_stride, jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views,
                                                float *h_matrices_out, int32_t *h_orient_out);
int jpeg_amd_decompress_tensor_projected_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                                               int n_images, int nthreads, int cosited, jpeg_amd_color color,
                                               const uint8_t *h_orient, const float *h_matrices,
                                               const jpeg_amd_warp *warp, int32_t out_w, int32_t out_h,
                                               const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                               const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride,
                                               jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views,
                                               float *h_matrices_out, int32_t *h_orient_out);

/* ---- bicubic warp: the bicubic filter in the projective calls ----------------------------------------------------------------
 *
 * "warped resample" and "projective resample" blend four taps.  These calls take `int filter` behind `warp` (the view:
 * behind `m`): with JPEG_AMD_FILTER_BILINEAR each is, bit for bit and status for status, the call of "projective resample" it
 * is named after; with JPEG_AMD_FILTER_BICUBIC the 4 x 4 taps of the Keys cubic with a = -0.5 stand in the blend's place.  It
 * is the polynomial of "bicubic resample" with the same operation order, over FOUR FIXED taps per axis: NOT widened by the
 * scale (there is no one scale under a map) and NOT renormalised (the weights sum to 1 up to rounding, and nothing is clipped:
 * the edge modes supply the taps outside).  This is PIL's BICUBIC kernel as Image.transform / rotate and torchvision's
 * RandomRotation, RandomAffine and RandomPerspective with interpolation=BICUBIC apply it.  torch's
 * grid_sample(mode="bicubic") uses a = -0.75 and is a different filter, as "bicubic resample" says of its interpolate.
 * Only the projective forms take a filter: a last row (0, 0, 1) is the affine warp (below), and one division per pixel is
 * nothing beside 16 taps -- one entry point, not two.
 *
 * THE CONTRACT.  Every statement is ONE binary32 operation and nothing is contracted; xs, xc, yc, nx, ny, nw, rw are those
 * of "projective resample", then
 *     sx = nx * rw;   sx = sx - 0.5f;   sx = min(max(sx, -2.0f), (float)w + 1.0f)        (likewise sy with h)
 *     fx0 = floorf(sx);   x0 = (int)fx0;   fx = sx - fx0                                   (x0 in -2 .. w + 1; likewise y0, fy)
 *     columns x0 - 1, x0, x0 + 1, x0 + 2 at the distances  fx + 1.0f,  fx,  1.0f - fx,  2.0f - fx
 *     the weight of a distance x:   x < 1:  ((1.5f * x - 2.5f) * x) * x + 1.0f
 *                                   x < 2:  ((((x - 5.0f) * x + 8.0f) * x) - 4.0f) * -0.5f
 *                                   else 0.0f                                  ("bicubic resample"'s two lines, word for word)
 *     rows y0 - 1 .. y0 + 2 the same with fy
 *     per row j and channel:  r_j = ((wx0 * t_j0 + wx1 * t_j1) + wx2 * t_j2) + wx3 * t_j3   (a product, then a sum, ascending)
 *     v = ((wy0 * r_0 + wy1 * r_1) + wy2 * r_2) + wy3 * r_3
 *     out = (uint8)(int)(min(max(v, 0.0f), 255.0f) + 0.5f)
 * A tap outside the image is (float)fill[c] under JPEG_AMD_EDGE_FILL; under JPEG_AMD_EDGE_REPLICATE its indices are clamped
 * into the image -- of the same jpeg_amd_warp.  "tensor output" and the "colour stage" act on this byte.
 *
 * THE LIMITS and refusals are those of "projective resample": the source side is at most 2^24, the conditioning of the
 * denominator is unchanged.  There is no tap limit and no ENOSUP.  Under a map JPEG_AMD_FILTER_ANTIALIAS and every other
 * value of `filter` is EINVAL -- there is no widening under a map -- judged where the edge mode is judged.
 *
 * CONSEQUENCES.
 *   - Identity.  The identity at out = (w, h) gives the source bytes: sx = x exactly, fx = 0, the weights are exactly
 *     0, 1, 0, 0 (the cubic is 0 at 1 and at 2) and the sums add zeros.
 *   - Integer translation.  An integer translation gives the shifted bytes, and the fill or the replicated edge where they
 *     came from outside.
 *   - Quarter turn.  (0, 1, 0, -1, 0, h, 0, 0, 1) to (h, w) is the quarter turn, as a permutation of bytes.
 *   - Far outside under FILL.  A pixel none of whose 16 taps lies inside is the fill byte: the weights' sum differs from 1 by
 *     a few ulp and the fill is an integer of at most 255, so v rounds to it.  Where the clamp binds, the fraction is 0, the
 *     weights are exactly 0, 1, 0, 0 and the one tap that counts (column -2 or w + 1, row -2 or h + 1) is outside: the same
 *     byte.  The kernels load nothing for such pixels.
 *   - A last row (0, 0, 1): rw = 1 and sx = nx exactly, so the map is the affine one of m[0 .. 5] -- the bicubic affine warp.
 *   - filter = JPEG_AMD_FILTER_BILINEAR through these entry points is the existing call, bit for bit and status for status;
 *     the entry points of "projective resample" ARE these with that value. */
int jpeg_amd_project_filter_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                  const jpeg_amd_extent *h_extents, const float *h_matrices, const jpeg_amd_warp *warp,
                                  int filter, int32_t out_w, int32_t out_h, uint8_t *d_dst, size_t dst_stride);
int jpeg_amd_project_filter_tensor_batch(jpeg_amd_ctx *ctx, int n_images, const uint8_t *d_src, size_t src_stride,
                                         const jpeg_amd_extent *h_extents, const float *h_matrices,
                                         const jpeg_amd_warp *warp, int filter, int32_t out_w, int32_t out_h,
                                         const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                         const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride);

/* jpeg_amd_project_view for a filter.  With JPEG_AMD_FILTER_BILINEAR it returns exactly what jpeg_amd_project_view returns.
 * With JPEG_AMD_FILTER_BICUBIC the footprint's margin (step 4) is one pixel wider on each side, since the taps reach
 * x0 - 1 .. x0 + 2: the view's columns are clamp(floor(xmin - 0.5) - 2, 0, W' - 1) ..= clamp(floor(xmax - 0.5) + 3, 0, W' - 1),
 * its rows likewise.  The denominator rule (step 2) and everything else are unchanged, and the one-pixel margin beyond the
 * taps covers the same rounding.  Any other filter is EINVAL. */
int jpeg_amd_project_filter_view(const jpeg_amd_layout *layout, int orientation, const float m[9], int filter, int32_t out_w,
                                 int32_t out_h, jpeg_amd_view *view, float m_view[9]);

/* The decode and file routes, by reference only: each is the *_projected_mixed call of the same place with views from
 * jpeg_amd_project_filter_view, and image i is, bit for bit, jpeg_amd_project_filter_batch (or the tensor form) applied to the
 * pixels jpeg_amd_decode_view_batch defines for the view jpeg_amd_project_filter_view returns, with the m_view it returns. */
int jpeg_amd_decode_projected_filter_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                           jpeg_amd_color color, const uint8_t *h_orient, const float *h_matrices,
                                           const jpeg_amd_warp *warp, int filter, int32_t out_w, int32_t out_h,
                                           jpeg_amd_view *h_views_out, float *h_matrices_out, uint8_t *d_pixels,
                                           size_t pixel_stride);
int jpeg_amd_decode_tensor_projected_filter_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited,
                                                  jpeg_amd_color color, const uint8_t *h_orient, const float *h_matrices,
                                                  const jpeg_amd_warp *warp, int filter, int32_t out_w, int32_t out_h,
                                                  const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                                  jpeg_amd_view *h_views_out, float *h_matrices_out,
                                                  const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride);
int jpeg_amd_decompress_resized_projected_filter_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                                                       int n_images, int nthreads, int cosited, jpeg_amd_color color,
                                                       const uint8_t *h_orient, const float *h_matrices,
                                                       const jpeg_amd_warp *warp, int filter, int32_t out_w, int32_t out_h,
                                                       uint8_t *d_pixels, size_t pixel_stride, jpeg_amd_frame_info *h_info,
                                                       jpeg_amd_view *h_views, float *h_matrices_out, int32_t *h_orient_out);
int jpeg_amd_decompress_tensor_projected_filter_mixed(jpeg_amd_ctx *ctx, const uint8_t *const h_jpeg[], const size_t nbytes[],
                                                      int n_images, int nthreads, int cosited, jpeg_amd_color color,
                                                      const uint8_t *h_orient, const float *h_matrices,
                                                      const jpeg_amd_warp *warp, int filter, int32_t out_w, int32_t out_h,
                                                      const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip,
                                                      const jpeg_amd_colour *colour, void *d_dst, size_t dst_stride,
                                                      jpeg_amd_frame_info *h_info, jpeg_amd_view *h_views,
                                                      float *h_matrices_out, int32_t *h_orient_out);

#ifdef __cplusplus
}
#endif
#endif /* JPEG_AMD_H */
