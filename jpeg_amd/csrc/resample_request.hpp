// resample_request.hpp -- what the caller of a resample call asked for, as one record: the entry points of capi_view.hip and
// capi_files.hip each build one, naming the fields they set, and the internal routes, declared at the end, take it by
// reference.  Host text only, nothing but the public header behind it: a stand-alone program can include it.
#pragma once

#include <cstddef>
#include <cstdint>

#include "jpeg_amd.h"

namespace jpeg_amd {
namespace capi {

// The map between the canvas and the source: none (the resize, with or without orientations and a placement), the affine map
// of the "warped resample" (6 numbers per image) or the homography of the "projective resample" (9).
enum class ResampleMap { None, Affine, Projective };

struct ResampleRequest {
    int32_t out_w = 0, out_h = 0;                     // the canvas
    int filter = JPEG_AMD_FILTER_BILINEAR;            // JPEG_AMD_FILTER_*; with a map ("bicubic warp"): bilinear, or bicubic with a projective one
    // the target: bytes, or the elements of a tensor.  `tensor` is not `spec != nullptr`: a tensor call without a spec is
    // jpeg_amd_tensor_extent's to refuse
    bool tensor = false;
    const jpeg_amd_tensor_spec *spec = nullptr;
    const uint8_t *h_flip = nullptr;                  // per image, or nullptr: none is mirrored
    void *d_dst = nullptr;
    size_t stride = 0;                                // between images, in elements
    const uint8_t *h_orient = nullptr;                // per image, or nullptr: every image as it is stored
    const jpeg_amd_placement *place = nullptr;        // or nullptr: every image fills the canvas
    jpeg_amd_region *h_windows_out = nullptr;         // per image, or nullptr: where a placed call writes its windows
    // with a map: per image matrix_floats() numbers against the image AS IT IS STORED at the launch's source (of a view:
    // map_view's m_view), and the call's warp
    ResampleMap map = ResampleMap::None;
    const float *h_matrices = nullptr;
    const jpeg_amd_warp *warp = nullptr;
    const jpeg_amd_colour *colour = nullptr;          // or nullptr: no colour stage

    static ResampleRequest bytes(int32_t out_w, int32_t out_h, void *d_pixels, size_t pixel_stride)
    {
        ResampleRequest r;
        r.out_w = out_w;
        r.out_h = out_h;
        r.d_dst = d_pixels;
        r.stride = pixel_stride;
        return r;
    }
    static ResampleRequest elements(int32_t out_w, int32_t out_h, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst,
                                    size_t dst_stride)
    {
        ResampleRequest r = bytes(out_w, out_h, d_dst, dst_stride);
        r.tensor = true;
        r.spec = spec;
        r.h_flip = h_flip;
        return r;
    }
    ResampleRequest &through(int filter_) { filter = filter_; return *this; }
    ResampleRequest &oriented(const uint8_t *h_orient_) { h_orient = h_orient_; return *this; }
    ResampleRequest &placed(const jpeg_amd_placement *place_, jpeg_amd_region *h_windows_out_)
    {
        place = place_;
        h_windows_out = h_windows_out_;
        return *this;
    }
    ResampleRequest &mapped(ResampleMap map_, const float *h_matrices_, const jpeg_amd_warp *warp_)
    {
        map = map_;
        h_matrices = h_matrices_;
        warp = warp_;
        return *this;
    }
    ResampleRequest &coloured(const jpeg_amd_colour *colour_) { colour = colour_; return *this; }

    bool has_map() const { return map != ResampleMap::None; }
    size_t matrix_floats() const { return map == ResampleMap::Projective ? 9 : 6; }
    // of a target that jpeg_amd_tensor_extent has passed
    size_t element_bytes() const { return !tensor ? 1 : spec->dtype == JPEG_AMD_F32 ? 4 : 2; }

    // Images [i0, i0 + m) of a checked call as a request of their own: every per-image array from image i0, the destination
    // from image i0's.  `room` holds the placement and the colour of the part, which point into the call's.
    struct Room {
        jpeg_amd_placement place;
        jpeg_amd_colour colour;
    };
    ResampleRequest images(int i0, int /* m: no array of the request carries its length */, Room *room) const
    {
        const size_t at = (size_t)i0;
        ResampleRequest r = *this;
        r.d_dst = static_cast<char *>(d_dst) + at * stride * element_bytes();
        if (h_flip) r.h_flip = h_flip + at;
        if (h_orient) r.h_orient = h_orient + at;
        if (h_windows_out) r.h_windows_out = h_windows_out + at;
        if (h_matrices) r.h_matrices = h_matrices + matrix_floats() * at;
        if (place) {
            room->place = *place;
            if (place->h_windows) room->place.h_windows = place->h_windows + at;
            r.place = &room->place;
        }
        if (colour) {
            room->colour = *colour;
            if (colour->h_matrices) room->colour.h_matrices = colour->h_matrices + 12 * at;
            r.colour = &room->colour;
        }
        return r;
    }
};


// The view that the map of `rq` reads of one image, and the matrix against it: jpeg_amd_warp_view's, or
// jpeg_amd_project_filter_view's at the request's filter.  For the mixed calls and for pass 0 of the file calls (capi_view.hip).
int map_view(const ResampleRequest &rq, const jpeg_amd_layout *layout, int orientation, const float *m, jpeg_amd_view *view, float *m_view);
// What the mixed resample calls (jpeg_amd_decode_resized_placed_mixed, jpeg_amd_decode_tensor_colour_mixed, ...) refuse of the
// request `rq` before they look at the context, for the file calls, which judge a call before its planes exist (the images'
// pointers only have to be non-null): of the first `judged` images of a call of n_images, in the mixed call's order; *taps:
// with judged == n_images the verdict on the antialiasing filter's tap limit, which that call gives last (capi_view.hip).
// With a map, rq.h_matrices are the matrices against the views.
int check_resampled_mixed(int n_images, int judged, const jpeg_amd_image *h_images, int cosited, jpeg_amd_color color,
                          const jpeg_amd_view *h_views, const ResampleRequest &rq, int *taps);
// The route of every mixed resample call behind its views: the views of the images, decoded chunk by chunk, resampled as `rq`
// says.  For the file calls, whose pass 0 has taken every file's view -- and, with a map, its m_view -- already (capi_view.hip).
int decode_views_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited, jpeg_amd_color color,
                       const jpeg_amd_view *h_views, const ResampleRequest &rq);

}  // namespace capi
}  // namespace jpeg_amd
