// colour_byte_target_test.cpp -- the one refusal of the "colour stage" that no public call reaches: a colour on a BYTE
// target.  The six *_colour_* entry points are tensor calls, but the internal routes they share with the byte calls take a
// colour and a `tensor` flag side by side: check_resampled_mixed (what the file calls judge before their planes exist) and
// decode_warped_views_mixed, both of jpeg_amd::capi (csrc/capi_internal.hpp), both with external linkage, neither needing a
// context or a device for what is judged here.  They are declared below as that header declares them -- the mangled name
// carries the parameter types, so a declaration that has drifted fails to link -- and called with a colour that is valid:
//   - tensor = false: EINVAL, for a call of no images (so before any image is looked at) and for one with images;
//   - the same arguments without the colour: OK -- the colour was what was refused;
//   - the same arguments with tensor = true: OK, and ENOSUP in *taps where the antialiasing filter's tap limit is passed.
// Links against libjpeg_amd.so; prints "ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "jpeg_amd.h"

namespace jpeg_amd {
namespace capi {
int check_resampled_mixed(int n_images, int judged, const jpeg_amd_image *h_images, int cosited, jpeg_amd_color color,
                          const jpeg_amd_view *h_views, int32_t out_w, int32_t out_h, int filter, const jpeg_amd_tensor_spec *spec,
                          bool tensor, const uint8_t *h_orient, const jpeg_amd_placement *place, void *d_dst, size_t dst_stride,
                          int *taps, const float *h_view_matrices, const jpeg_amd_warp *warp, bool warped, const jpeg_amd_colour *colour);
int decode_warped_views_mixed(jpeg_amd_ctx *ctx, int n_images, const jpeg_amd_image *h_images, int cosited, jpeg_amd_color color,
                              const jpeg_amd_view *h_views, const float *h_view_matrices, const jpeg_amd_warp *warp, int32_t out_w,
                              int32_t out_h, bool tensor, const jpeg_amd_tensor_spec *spec, const uint8_t *h_flip, void *d_dst,
                              size_t dst_stride, const jpeg_amd_colour *colour);
}  // namespace capi
}  // namespace jpeg_amd

using namespace jpeg_amd::capi;

#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("line %d: %s\n", __LINE__, #cond);                    \
            return 1;                                                         \
        }                                                                     \
    } while (0)

int main()
{
    constexpr int N = 2;
    void *const ptr = reinterpret_cast<void *>(0x1000);   // a device pointer that is never followed
    jpeg_amd_image images[N] = {};
    jpeg_amd_view views[N];
    const int32_t side = 400;
    for (int i = 0; i < N; ++i) {
        jpeg_amd_layout &L = images[i].layout;
        L.width = L.height = side;
        L.precision = 8;
        L.nplanes = 3;
        L.scale_x = L.scale_y = 1;
        for (int p = 0; p < 3; ++p) {
            L.factor_x[p] = L.factor_y[p] = 1;
            L.qi[p] = p ? 1 : 0;
            images[i].d_coef[p] = static_cast<const int16_t *>(ptr);
        }
        EXPECT(jpeg_amd_layout_units(&L) == JPEG_AMD_OK);
        images[i].d_quanta = static_cast<const uint16_t *>(ptr);
        images[i].ntables = 2;
        views[i] = jpeg_amd_view{1, jpeg_amd_region{0, 0, side, side}};
    }
    const float k[N][12] = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, {0, 0, 1, 5, 0, 1, 0, 0, 1, 0, 0, -5}};
    const jpeg_amd_colour colour{&k[0][0], 0.0f, 255.0f}, free_colour{&k[0][0], -INFINITY, INFINITY};
    const jpeg_amd_tensor_spec spec{JPEG_AMD_F32, JPEG_AMD_TENSOR_CHW, {0, 0, 0}, {1, 1, 1}};
    const size_t stride = 3 * 64 * 64;

    // ---- check_resampled_mixed: the placed route
    for (const jpeg_amd_colour *c : {&colour, &free_colour}) {
        for (const int n : {0, N}) {
            for (const int filter : {JPEG_AMD_FILTER_BILINEAR, JPEG_AMD_FILTER_ANTIALIAS}) {
                int taps = -99;
                // bytes with a colour: refused, whatever else the call holds
                EXPECT(check_resampled_mixed(n, n, images, 0, JPEG_AMD_COLOR_RGB8, views, 64, 64, filter, nullptr, false, nullptr, nullptr, ptr,
                                             stride, &taps, nullptr, nullptr, false, c) == JPEG_AMD_EINVAL);
                EXPECT(check_resampled_mixed(n, n, images, 0, JPEG_AMD_COLOR_RGB8, views, 64, 64, filter, &spec, false, nullptr, nullptr, ptr,
                                             stride, &taps, nullptr, nullptr, false, c) == JPEG_AMD_EINVAL);
                EXPECT(taps == -99);
                // bytes without one, and a tensor with one: judged to the end
                EXPECT(check_resampled_mixed(n, n, images, 0, JPEG_AMD_COLOR_RGB8, views, 64, 64, filter, nullptr, false, nullptr, nullptr, ptr,
                                             stride, &taps, nullptr, nullptr, false, nullptr) == JPEG_AMD_OK);
                EXPECT(taps == JPEG_AMD_OK);
                taps = -99;
                EXPECT(check_resampled_mixed(n, n, images, 0, JPEG_AMD_COLOR_RGB8, views, 64, 64, filter, &spec, true, nullptr, nullptr, ptr,
                                             stride, &taps, nullptr, nullptr, false, c) == JPEG_AMD_OK);
                EXPECT(taps == JPEG_AMD_OK);
            }
        }
        // 400 x 400 to 8 x 8 through the antialiasing filter is a scale of 50: the tap limit, behind the colour
        int taps = -99;
        EXPECT(check_resampled_mixed(N, N, images, 0, JPEG_AMD_COLOR_RGB8, views, 8, 8, JPEG_AMD_FILTER_ANTIALIAS, &spec, true, nullptr, nullptr,
                                     ptr, 3 * 8 * 8, &taps, nullptr, nullptr, false, c) == JPEG_AMD_OK);
        EXPECT(taps == JPEG_AMD_ENOSUP);
        taps = -99;
        EXPECT(check_resampled_mixed(N, N, images, 0, JPEG_AMD_COLOR_RGB8, views, 8, 8, JPEG_AMD_FILTER_ANTIALIAS, nullptr, false, nullptr, nullptr,
                                     ptr, 3 * 8 * 8, &taps, nullptr, nullptr, false, c) == JPEG_AMD_EINVAL);
        EXPECT(taps == -99);
    }

    // ---- the warped route, both functions: a call of no images needs no context
    const jpeg_amd_warp warp{JPEG_AMD_EDGE_FILL, {1, 2, 3}};
    const float m[N][6] = {{1, 0, 0, 0, 1, 0}, {1, 0, 0, 0, 1, 0}};
    for (const int n : {0, N}) {
        int taps = -99;
        EXPECT(check_resampled_mixed(n, n, images, 0, JPEG_AMD_COLOR_RGB8, views, 64, 64, JPEG_AMD_FILTER_BILINEAR, nullptr, false, nullptr,
                                     nullptr, ptr, stride, &taps, &m[0][0], &warp, true, &colour) == JPEG_AMD_EINVAL);
        EXPECT(check_resampled_mixed(n, n, images, 0, JPEG_AMD_COLOR_RGB8, views, 64, 64, JPEG_AMD_FILTER_BILINEAR, nullptr, false, nullptr,
                                     nullptr, ptr, stride, &taps, &m[0][0], &warp, true, nullptr) == JPEG_AMD_OK);
        EXPECT(check_resampled_mixed(n, n, images, 0, JPEG_AMD_COLOR_RGB8, views, 64, 64, JPEG_AMD_FILTER_BILINEAR, &spec, true, nullptr,
                                     nullptr, ptr, stride, &taps, &m[0][0], &warp, true, &colour) == JPEG_AMD_OK);
    }
    EXPECT(decode_warped_views_mixed(nullptr, 0, images, 0, JPEG_AMD_COLOR_RGB8, views, &m[0][0], &warp, 64, 64, false, nullptr, nullptr, ptr,
                                     stride, &colour) == JPEG_AMD_EINVAL);
    EXPECT(decode_warped_views_mixed(nullptr, 0, images, 0, JPEG_AMD_COLOR_RGB8, views, &m[0][0], &warp, 64, 64, false, nullptr, nullptr, ptr,
                                     stride, nullptr) == JPEG_AMD_OK);
    EXPECT(decode_warped_views_mixed(nullptr, 0, images, 0, JPEG_AMD_COLOR_RGB8, views, &m[0][0], &warp, 64, 64, true, &spec, nullptr, ptr,
                                     stride, &colour) == JPEG_AMD_OK);
    // with images the byte call with a colour is refused in front of the context (NULL here), which a right call reaches
    EXPECT(decode_warped_views_mixed(nullptr, N, images, 0, JPEG_AMD_COLOR_RGB8, views, &m[0][0], &warp, 64, 64, false, nullptr, nullptr, ptr,
                                     stride, &colour) == JPEG_AMD_EINVAL);
    std::printf("ok\n");
    return 0;
}
