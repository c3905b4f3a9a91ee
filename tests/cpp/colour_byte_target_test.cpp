// colour_byte_target_test.cpp -- the one refusal of the "colour stage" that no public call reaches: a colour on a BYTE
// target.  The six *_colour_* entry points are tensor calls, but the internal routes they share with the byte calls take a
// request (csrc/resample_request.hpp) that holds a colour and a `tensor` flag side by side: check_resampled_mixed (what the
// file calls judge before their planes exist) and decode_views_mixed, both of jpeg_amd::capi, both with external linkage,
// neither needing a context or a device for what is judged here.  That header declares them -- the mangled name carries the
// parameter types, so a definition that has drifted fails to link -- and they are called with a colour that is valid:
//   - a byte target: EINVAL, for a call of no images (so before any image is looked at) and for one with images;
//   - the same request without the colour: OK -- the colour was what was refused;
//   - the same request to a tensor: OK, and ENOSUP in *taps where the antialiasing filter's tap limit is passed.
// Without a map, through the affine map and through the projective one.  Links against libjpeg_amd.so; prints "ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "resample_request.hpp"

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
    const auto check = [&](int n, const ResampleRequest &rq, int *taps) {
        return check_resampled_mixed(n, n, images, 0, JPEG_AMD_COLOR_RGB8, views, rq, taps);
    };
    // a byte target that carries a spec all the same: `tensor` decides, not the spec
    const auto bytes_with_spec = [&](int32_t w, int32_t h, size_t s) {
        ResampleRequest rq = ResampleRequest::bytes(w, h, ptr, s);
        rq.spec = &spec;
        return rq;
    };

    // ---- check_resampled_mixed: the placed route
    for (const jpeg_amd_colour *c : {&colour, &free_colour}) {
        for (const int n : {0, N}) {
            for (const int filter : {JPEG_AMD_FILTER_BILINEAR, JPEG_AMD_FILTER_ANTIALIAS}) {
                int taps = -99;
                // bytes with a colour: refused, whatever else the call holds
                EXPECT(check(n, ResampleRequest::bytes(64, 64, ptr, stride).through(filter).coloured(c), &taps) == JPEG_AMD_EINVAL);
                EXPECT(check(n, bytes_with_spec(64, 64, stride).through(filter).coloured(c), &taps) == JPEG_AMD_EINVAL);
                EXPECT(taps == -99);
                // bytes without one, and a tensor with one: judged to the end
                EXPECT(check(n, ResampleRequest::bytes(64, 64, ptr, stride).through(filter), &taps) == JPEG_AMD_OK);
                EXPECT(taps == JPEG_AMD_OK);
                taps = -99;
                EXPECT(check(n, ResampleRequest::elements(64, 64, &spec, nullptr, ptr, stride).through(filter).coloured(c), &taps) ==
                       JPEG_AMD_OK);
                EXPECT(taps == JPEG_AMD_OK);
            }
        }
        // 400 x 400 to 8 x 8 through the antialiasing filter is a scale of 50: the tap limit, behind the colour
        int taps = -99;
        EXPECT(check(N, ResampleRequest::elements(8, 8, &spec, nullptr, ptr, 3 * 8 * 8).through(JPEG_AMD_FILTER_ANTIALIAS).coloured(c),
                     &taps) == JPEG_AMD_OK);
        EXPECT(taps == JPEG_AMD_ENOSUP);
        taps = -99;
        EXPECT(check(N, ResampleRequest::bytes(8, 8, ptr, 3 * 8 * 8).through(JPEG_AMD_FILTER_ANTIALIAS).coloured(c), &taps) ==
               JPEG_AMD_EINVAL);
        EXPECT(taps == -99);
    }

    // ---- the routes through a map, both functions, affine and projective: a call of no images needs no context
    const jpeg_amd_warp warp{JPEG_AMD_EDGE_FILL, {1, 2, 3}};
    const float m6[N][6] = {{1, 0, 0, 0, 1, 0}, {1, 0, 0, 0, 1, 0}};
    const float m9[N][9] = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {1, 0, 0, 0, 1, 0, 0, 0, 1}};
    for (const ResampleMap map : {ResampleMap::Affine, ResampleMap::Projective}) {
        const float *m = map == ResampleMap::Affine ? &m6[0][0] : &m9[0][0];
        const ResampleRequest bytes = ResampleRequest::bytes(64, 64, ptr, stride).mapped(map, m, &warp);
        const ResampleRequest elements = ResampleRequest::elements(64, 64, &spec, nullptr, ptr, stride).mapped(map, m, &warp);
        for (const int n : {0, N}) {
            int taps = -99;
            EXPECT(check(n, ResampleRequest(bytes).coloured(&colour), &taps) == JPEG_AMD_EINVAL);
            EXPECT(check(n, bytes, &taps) == JPEG_AMD_OK);
            EXPECT(check(n, ResampleRequest(elements).coloured(&colour), &taps) == JPEG_AMD_OK);
        }
        EXPECT(decode_views_mixed(nullptr, 0, images, 0, JPEG_AMD_COLOR_RGB8, views, ResampleRequest(bytes).coloured(&colour)) ==
               JPEG_AMD_EINVAL);
        EXPECT(decode_views_mixed(nullptr, 0, images, 0, JPEG_AMD_COLOR_RGB8, views, bytes) == JPEG_AMD_OK);
        EXPECT(decode_views_mixed(nullptr, 0, images, 0, JPEG_AMD_COLOR_RGB8, views, ResampleRequest(elements).coloured(&colour)) ==
               JPEG_AMD_OK);
        // with images the byte call with a colour is refused in front of the context (NULL here), which a right call reaches
        EXPECT(decode_views_mixed(nullptr, N, images, 0, JPEG_AMD_COLOR_RGB8, views, ResampleRequest(bytes).coloured(&colour)) ==
               JPEG_AMD_EINVAL);
    }
    std::printf("ok\n");
    return 0;
}
