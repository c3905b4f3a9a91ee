"""ctypes binding of include/jpeg_amd.h.  There is NO fallback: if the HIP library is
missing or a call fails, this raises."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# JPEG_AMD_LIBRARY points at an alternative build of the same library (tools/ experiments)
LIB_PATH = os.environ.get("JPEG_AMD_LIBRARY") or os.path.join(HERE, "libjpeg_amd.so")
MAX_PLANES = 4

OK, EINVAL, ENOMEM, EHIP, ENODEV, ENOSUP = 0, -1, -2, -3, -4, -5
COLOR_YCC8, COLOR_RGB8 = 0, 1
CTX_OWN_STREAM = 1
CTX_DEVICE_ENTROPY = 2


class JpegAmdError(RuntimeError):
    def __init__(self, status: int, what: str, hip: int = 0):
        self.status, self.hip = status, hip
        msg = lib().jpeg_amd_strerror(status).decode()
        super().__init__(f"{what}: {msg} (status {status}" + (f", hipError {hip})" if hip else ")"))


class Layout(C.Structure):
    """struct jpeg_amd_layout"""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("precision", C.c_int32),
        ("nplanes", C.c_int32), ("scale_x", C.c_int32), ("scale_y", C.c_int32),
        ("factor_x", C.c_int32 * MAX_PLANES), ("factor_y", C.c_int32 * MAX_PLANES),
        ("units_x", C.c_int32 * MAX_PLANES), ("units_y", C.c_int32 * MAX_PLANES),
        ("qi", C.c_int32 * MAX_PLANES),
    ]


_p = C.c_void_p
_pp = C.POINTER(C.c_void_p)
_szp = C.POINTER(C.c_size_t)
_L = C.POINTER(Layout)

# name -> (restype, argtypes); mirrors include/jpeg_amd.h one to one
SIGNATURES = {
    "jpeg_amd_version": (C.c_int, []),
    "jpeg_amd_strerror": (C.c_char_p, [C.c_int]),
    "jpeg_amd_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "jpeg_amd_ctx_create": (C.c_int, [C.c_int, _p, C.c_int, _pp]),
    "jpeg_amd_ctx_destroy": (C.c_int, [_p]),
    "jpeg_amd_ctx_synchronize": (C.c_int, [_p]),
    "jpeg_amd_last_hip_error": (C.c_int, [_p]),
    "jpeg_amd_layout_units": (C.c_int, [_L]),
    "jpeg_amd_malloc": (C.c_int, [_p, C.c_size_t, _pp]),
    "jpeg_amd_free": (C.c_int, [_p, _p]),
    "jpeg_amd_memcpy_h2d": (C.c_int, [_p, _p, _p, C.c_size_t]),
    "jpeg_amd_memcpy_d2h": (C.c_int, [_p, _p, _p, C.c_size_t]),
    "jpeg_amd_timer_begin": (C.c_int, [_p]),
    "jpeg_amd_timer_end": (C.c_int, [_p, C.POINTER(C.c_float)]),
    "jpeg_amd_idct_plane": (C.c_int, [_p, _p, C.c_int, C.c_int, _p, C.c_int, _p]),
    "jpeg_amd_spectral_idct": (C.c_int, [_p, _L, _pp, _p, C.c_int, _pp]),
    "jpeg_amd_planar_interleaved": (C.c_int, [_p, _L, _pp, C.c_int, _p]),
    "jpeg_amd_rectangular_unpack": (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_int, _p]),
    "jpeg_amd_decode_batch": (C.c_int, [_p, _L, C.c_int, _pp, _szp, _p, C.c_size_t, C.c_int,
                                        C.c_int, C.c_int, _p, C.c_size_t]),
    "jpeg_amd_decode": (C.c_int, [_p, _L, _pp, _p, C.c_int, C.c_int, C.c_int, _p]),
    "jpeg_amd_spectral_rectangular_batch": (C.c_int, [_p, _L, C.c_int, _pp, _szp, _p, C.c_size_t, C.c_int, C.c_int, _p, C.c_size_t]),
    "jpeg_amd_spectral_rectangular": (C.c_int, [_p, _L, _pp, _p, C.c_int, C.c_int, _p]),
    "jpeg_amd_host_spectral_rectangular": (C.c_int, [_p, _L, _pp, _p, C.c_int, C.c_int, _p]),
    "jpeg_amd_rectangular_spectral_batch": (C.c_int, [_p, _L, C.c_int, _p, C.c_size_t, _p, C.c_size_t, C.c_int, _pp, _szp]),
    "jpeg_amd_rectangular_spectral": (C.c_int, [_p, _L, _p, _p, C.c_int, _pp]),
    "jpeg_amd_host_rectangular_spectral": (C.c_int, [_p, _L, _p, _p, C.c_int, _pp]),
    "jpeg_amd_rectangular_pack": (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_int, _p]),
    "jpeg_amd_rectangular_decomposed": (C.c_int, [_p, _L, _p, _pp]),
    "jpeg_amd_fdct_plane": (C.c_int, [_p, _p, C.c_int, C.c_int, _p, C.c_int, _p]),
    "jpeg_amd_planar_fdct": (C.c_int, [_p, _L, _pp, _p, C.c_int, _pp]),
    "jpeg_amd_encode_batch": (C.c_int, [_p, _L, C.c_int, _p, C.c_size_t, C.c_int, _p,
                                        C.c_size_t, C.c_int, _pp, _szp]),
    "jpeg_amd_encode": (C.c_int, [_p, _L, _p, C.c_int, _p, C.c_int, _pp]),
    "jpeg_amd_host_spectral_idct": (C.c_int, [_p, _L, _pp, _p, C.c_int, _pp]),
    "jpeg_amd_host_planar_interleaved": (C.c_int, [_p, _L, _pp, C.c_int, _p]),
    "jpeg_amd_host_rectangular_unpack": (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_int, _p]),
    "jpeg_amd_host_decode": (C.c_int, [_p, _L, _pp, _p, C.c_int, C.c_int, C.c_int, _p]),
    "jpeg_amd_host_rectangular_pack": (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_int, _p]),
    "jpeg_amd_host_rectangular_decomposed": (C.c_int, [_p, _L, _p, _pp]),
    "jpeg_amd_host_planar_fdct": (C.c_int, [_p, _L, _pp, _p, C.c_int, _pp]),
    "jpeg_amd_host_encode": (C.c_int, [_p, _L, _p, C.c_int, _p, C.c_int, _pp]),
    "jpeg_amd_huffman_lookup": (C.c_int, [_p, _p, C.c_int, C.c_uint16, _p, _p]),
    "jpeg_amd_huffman_build": (C.c_int, [_p, _p, _p, _p]),
    "jpeg_amd_jpeg_inspect": (C.c_int, [_p, C.c_size_t, _p]),
    "jpeg_amd_jpeg_decode_spectral": (C.c_int, [_p, C.c_size_t, _pp, _p, _p]),
    "jpeg_amd_jpeg_decode_spectral_mt": (C.c_int, [_p, C.c_size_t, _pp, _p, _p, C.c_int]),
    "jpeg_amd_jpeg_decode_spectral_partial": (C.c_int, [_p, C.c_size_t, _pp, _p, _p, C.c_int, C.c_int]),
    "jpeg_amd_spectral_expand_batch": (C.c_int, [_p, _L, C.c_int, _p, C.c_size_t, _p, C.c_size_t, _p, _pp, _szp]),
    "jpeg_amd_spectral_sparsify_batch": (C.c_int, [_p, _L, C.c_int, _pp, _szp, _p, C.c_size_t, _p, C.c_size_t, C.c_uint32, _p]),
    "jpeg_amd_jpeg_decode_sparse": (C.c_int, [_p, C.c_size_t, _p, C.c_size_t, _p, C.c_size_t, _p, _p, _p]),
    "jpeg_amd_jpeg_plan_intervals": (C.c_int, [_p, C.c_size_t, _p, _p, _p]),
    "jpeg_amd_jpeg_decode_intervals_host": (C.c_int, [_p, C.c_size_t, _pp, _p, _p]),
    "jpeg_amd_jpeg_decode_spectral_device": (C.c_int, [_p, C.c_int, _pp, _szp, _p, _p, _p, _p]),
    "jpeg_amd_ctx_device_entropy_files": (C.c_int, [_p, _p]),
    "jpeg_amd_ctx_device_entropy_kernel_ms": (C.c_int, [_p, _p]),
    "jpeg_amd_stream_create": (C.c_void_p, []),
    "jpeg_amd_stream_destroy": (None, [_p]),
    "jpeg_amd_stream_push": (C.c_int, [_p, _p, C.c_size_t, _p, _p]),
    "jpeg_amd_stream_info": (C.c_int, [_p, _p]),
    "jpeg_amd_stream_snapshot": (C.c_int, [_p, _pp, _p]),
    "jpeg_amd_decompress": (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_int, _p, C.c_size_t, _p]),
    "jpeg_amd_decompress_rectangular": (C.c_int, [_p, _p, C.c_size_t, C.c_int, C.c_int, C.c_int, _p, C.c_size_t, _p]),
    "jpeg_amd_decompress_batch": (C.c_int, [_p, _pp, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, C.c_size_t, _p]),
    "jpeg_amd_decompress_batch_device": (C.c_int, [_p, _pp, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, C.c_size_t, _p]),
    "jpeg_amd_jpeg_encode_spectral": (C.c_int, [_p, _p, _pp, _p, _p, C.c_int, _p, C.c_int, _p, C.c_int, _p, C.c_size_t, _p]),
    "jpeg_amd_jpeg_encode_sparse": (C.c_int, [_p, _p, _p, _p, C.c_size_t, _p, _p, C.c_int, _p, C.c_int, _p, C.c_int, _p, C.c_size_t, _p]),
    "jpeg_amd_compress": (C.c_int, [_p, _p, _p, C.c_int, _p, _p, _p, C.c_int, _p, C.c_int, _p, C.c_int, _p, C.c_size_t, _p]),
    "jpeg_amd_compress_rectangular": (C.c_int, [_p, _p, _p, _p, _p, _p, C.c_int, _p, C.c_int, _p, C.c_int, _p, C.c_size_t, _p]),
    "jpeg_amd_compress_batch": (C.c_int, [_p, _p, _p, C.c_size_t, C.c_int, C.c_int, _p, _p, _p, C.c_int, _p, C.c_int, _p, C.c_int,
                                          C.c_int, _p, C.c_size_t, _p]),
    "jpeg_amd_compress_batch_device": (C.c_int, [_p, _p, _p, C.c_size_t, C.c_int, C.c_int, _p, _p, _p, C.c_int, _p, C.c_int, _p, C.c_int,
                                                 C.c_int, _p, C.c_size_t, _p]),
    "jpeg_amd_transform_layout": (C.c_int, [_L, C.c_int, _p, _L]),
    "jpeg_amd_transform_quanta": (C.c_int, [C.c_int, _p, _p]),
    "jpeg_amd_spectral_transform_batch": (C.c_int, [_p, _L, C.c_int, C.c_int, _p, _pp, _szp, _p, C.c_size_t, C.c_int, _p, _pp, _szp,
                                                    _p]),
    "jpeg_amd_spectral_transform": (C.c_int, [_p, _L, C.c_int, _p, _pp, _p, C.c_int, _p, _pp]),
    "jpeg_amd_jpeg_script": (C.c_int, [_p, C.c_size_t, _p, C.c_int, _p, _p, _p, C.c_int, _p]),
    "jpeg_amd_transform": (C.c_int, [_p, _p, C.c_size_t, C.c_int, _p, _p, C.c_int, _p, C.c_size_t, _p, _p]),
    "jpeg_amd_decode_region_batch": (C.c_int, [_p, _L, C.c_int, _pp, _szp, _p, C.c_size_t, C.c_int, C.c_int, C.c_int, _p, _p,
                                               C.c_size_t]),
    "jpeg_amd_decode_region": (C.c_int, [_p, _L, _pp, _p, C.c_int, C.c_int, C.c_int, _p, _p]),
    "jpeg_amd_region_window": (C.c_int, [_L, C.c_int, _p, _p]),
    "jpeg_amd_decode_scaled_batch": (C.c_int, [_p, _L, C.c_int, _pp, _szp, _p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, _p,
                                               C.c_size_t]),
    "jpeg_amd_decode_scaled": (C.c_int, [_p, _L, _pp, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p]),
    "jpeg_amd_scaled_layout": (C.c_int, [_L, C.c_int, _L]),
    "jpeg_amd_spectral_idct_scaled": (C.c_int, [_p, _L, _pp, _p, C.c_int, C.c_int, _pp]),
    "jpeg_amd_decode_view_batch": (C.c_int, [_p, _L, C.c_int, _pp, _szp, _p, C.c_size_t, C.c_int, C.c_int, C.c_int, _p, _p,
                                             C.c_size_t]),
    "jpeg_amd_decode_view": (C.c_int, [_p, _L, _pp, _p, C.c_int, C.c_int, C.c_int, _p, _p]),
    "jpeg_amd_view_window": (C.c_int, [_L, C.c_int, C.c_int, _p, _p]),
    "jpeg_amd_view_of_source": (C.c_int, [_L, C.c_int, _p, _p]),
    "jpeg_amd_view_denom": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "jpeg_amd_resize_batch": (C.c_int, [_p, C.c_int, _p, C.c_size_t, _p, C.c_int32, C.c_int32, _p, C.c_size_t]),
    "jpeg_amd_decode_resized_batch": (C.c_int, [_p, _L, C.c_int, _pp, _szp, _p, C.c_size_t, C.c_int, C.c_int, C.c_int, _p, C.c_int32,
                                                C.c_int32, _p, C.c_size_t]),
    "jpeg_amd_decode_resized": (C.c_int, [_p, _L, _pp, _p, C.c_int, C.c_int, C.c_int, _p, C.c_int32, C.c_int32, _p]),
    "jpeg_amd_tensor_extent": (C.c_int, [_p, C.c_int32, C.c_int32, _szp, _szp]),
    "jpeg_amd_resize_tensor_batch": (C.c_int, [_p, C.c_int, _p, C.c_size_t, _p, C.c_int32, C.c_int32, _p, _p, _p, C.c_size_t]),
    "jpeg_amd_decode_tensor_batch": (C.c_int, [_p, _L, C.c_int, _pp, _szp, _p, C.c_size_t, C.c_int, C.c_int, C.c_int, _p, C.c_int32,
                                               C.c_int32, _p, _p, _p, C.c_size_t]),
    "jpeg_amd_decode_tensor": (C.c_int, [_p, _L, _pp, _p, C.c_int, C.c_int, C.c_int, _p, C.c_int32, C.c_int32, _p, C.c_int, _p]),
    "jpeg_amd_decode_view_mixed": (C.c_int, [_p, C.c_int, _p, C.c_int, C.c_int, _p, _p, C.c_size_t]),
    "jpeg_amd_decode_resized_mixed": (C.c_int, [_p, C.c_int, _p, C.c_int, C.c_int, _p, C.c_int32, C.c_int32, _p, C.c_size_t]),
    "jpeg_amd_decode_tensor_mixed": (C.c_int, [_p, C.c_int, _p, C.c_int, C.c_int, _p, C.c_int32, C.c_int32, _p, _p, _p, C.c_size_t]),
    "jpeg_amd_resize_filter_batch": (C.c_int, [_p, C.c_int, _p, C.c_size_t, _p, C.c_int32, C.c_int32, C.c_int, _p, C.c_size_t]),
    "jpeg_amd_resize_filter_tensor_batch": (C.c_int, [_p, C.c_int, _p, C.c_size_t, _p, C.c_int32, C.c_int32, C.c_int, _p, _p, _p,
                                                      C.c_size_t]),
    "jpeg_amd_decode_resized_filter_batch": (C.c_int, [_p, _L, C.c_int, _pp, _szp, _p, C.c_size_t, C.c_int, C.c_int, C.c_int, _p,
                                                       C.c_int32, C.c_int32, C.c_int, _p, C.c_size_t]),
    "jpeg_amd_decode_tensor_filter_batch": (C.c_int, [_p, _L, C.c_int, _pp, _szp, _p, C.c_size_t, C.c_int, C.c_int, C.c_int, _p,
                                                      C.c_int32, C.c_int32, C.c_int, _p, _p, _p, C.c_size_t]),
    "jpeg_amd_decode_resized_filter_mixed": (C.c_int, [_p, C.c_int, _p, C.c_int, C.c_int, _p, C.c_int32, C.c_int32, C.c_int, _p,
                                                       C.c_size_t]),
    "jpeg_amd_decode_tensor_filter_mixed": (C.c_int, [_p, C.c_int, _p, C.c_int, C.c_int, _p, C.c_int32, C.c_int32, C.c_int, _p, _p,
                                                      _p, C.c_size_t]),
    "jpeg_amd_tensor_source_extent": (C.c_int, [_p, C.c_int32, C.c_int32, _szp, _szp]),
    "jpeg_amd_tensor_pixels_batch": (C.c_int, [_p, C.c_int, _p, C.c_size_t, C.c_int32, C.c_int32, _p, _p, C.c_size_t]),
    "jpeg_amd_encode_tensor_batch": (C.c_int, [_p, _L, C.c_int, _p, C.c_size_t, _p, C.c_int, _p, C.c_size_t, C.c_int, _pp, _szp]),
    "jpeg_amd_encode_tensor": (C.c_int, [_p, _L, _p, _p, C.c_int, _p, C.c_int, _pp]),
    "jpeg_amd_compress_tensor_batch_device": (C.c_int, [_p, _p, _p, C.c_size_t, _p, C.c_int, C.c_int, _p, _p, _p, C.c_int, _p,
                                                        C.c_int, _p, C.c_int, C.c_int, _p, C.c_size_t, _p]),
    "jpeg_amd_reduce_layout": (C.c_int, [_L, C.c_int, _L]),
    "jpeg_amd_spectral_reduce_batch": (C.c_int, [_p, _L, C.c_int, C.c_int, _pp, _szp, _p, C.c_size_t, C.c_int, _p, _pp, _szp]),
    "jpeg_amd_spectral_reduce": (C.c_int, [_p, _L, C.c_int, _pp, _p, C.c_int, _p, _pp]),
    "jpeg_amd_reduce": (C.c_int, [_p, _p, C.c_size_t, C.c_int, _p, C.c_int, _p, C.c_size_t, _p, _p]),
    "jpeg_amd_spectral_expand_mixed": (C.c_int, [_p, C.c_int, _p, _p]),
    "jpeg_amd_decompress_tensor_mixed": (C.c_int, [_p, _pp, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, C.c_int32, C.c_int32, C.c_int,
                                                   _p, _p, _p, C.c_size_t, _p, _p]),
    "jpeg_amd_decompress_resized_mixed": (C.c_int, [_p, _pp, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, C.c_int32, C.c_int32, C.c_int,
                                                    _p, C.c_size_t, _p, _p]),
    "jpeg_amd_jpeg_orientation": (C.c_int, [_p, C.c_size_t, _p]),
    "jpeg_amd_orient_region": (C.c_int, [C.c_int, C.c_int32, C.c_int32, _p, _p]),
    "jpeg_amd_resize_oriented_batch": (C.c_int, [_p, C.c_int, _p, C.c_size_t, _p, C.c_int32, C.c_int32, C.c_int, _p, _p, C.c_size_t]),
    "jpeg_amd_resize_oriented_tensor_batch": (C.c_int, [_p, C.c_int, _p, C.c_size_t, _p, C.c_int32, C.c_int32, C.c_int, _p, _p, _p, _p,
                                                        C.c_size_t]),
    "jpeg_amd_decode_resized_oriented_mixed": (C.c_int, [_p, C.c_int, _p, C.c_int, C.c_int, _p, C.c_int32, C.c_int32, C.c_int, _p, _p,
                                                         C.c_size_t]),
    "jpeg_amd_decode_tensor_oriented_mixed": (C.c_int, [_p, C.c_int, _p, C.c_int, C.c_int, _p, C.c_int32, C.c_int32, C.c_int, _p, _p,
                                                        _p, _p, C.c_size_t]),
    "jpeg_amd_decompress_tensor_oriented_mixed": (C.c_int, [_p, _pp, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, C.c_int32, C.c_int32,
                                                            C.c_int, _p, _p, _p, _p, C.c_size_t, _p, _p, _p]),
    "jpeg_amd_decompress_resized_oriented_mixed": (C.c_int, [_p, _pp, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, C.c_int32, C.c_int32,
                                                             C.c_int, _p, _p, C.c_size_t, _p, _p, _p]),
    "jpeg_amd_place_window": (C.c_int, [C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _p]),
    "jpeg_amd_resize_placed_batch": (C.c_int, [_p, C.c_int, _p, C.c_size_t, _p, C.c_int32, C.c_int32, C.c_int, _p, _p, _p, _p,
                                               C.c_size_t]),
    "jpeg_amd_resize_placed_tensor_batch": (C.c_int, [_p, C.c_int, _p, C.c_size_t, _p, C.c_int32, C.c_int32, C.c_int, _p, _p, _p, _p,
                                                      _p, _p, C.c_size_t]),
    "jpeg_amd_decode_resized_placed_mixed": (C.c_int, [_p, C.c_int, _p, C.c_int, C.c_int, _p, C.c_int32, C.c_int32, C.c_int, _p, _p,
                                                       _p, _p, C.c_size_t]),
    "jpeg_amd_decode_tensor_placed_mixed": (C.c_int, [_p, C.c_int, _p, C.c_int, C.c_int, _p, C.c_int32, C.c_int32, C.c_int, _p, _p,
                                                      _p, _p, _p, _p, C.c_size_t]),
    "jpeg_amd_decompress_tensor_placed_mixed": (C.c_int, [_p, _pp, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, C.c_int32, C.c_int32,
                                                          C.c_int, _p, _p, _p, _p, _p, _p, C.c_size_t, _p, _p, _p]),
    "jpeg_amd_decompress_resized_placed_mixed": (C.c_int, [_p, _pp, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, C.c_int32, C.c_int32,
                                                           C.c_int, _p, _p, _p, _p, C.c_size_t, _p, _p, _p]),
    "jpeg_amd_warp_batch": (C.c_int, [_p, C.c_int, _p, C.c_size_t, _p, _p, _p, C.c_int32, C.c_int32, _p, C.c_size_t]),
    "jpeg_amd_warp_tensor_batch": (C.c_int, [_p, C.c_int, _p, C.c_size_t, _p, _p, _p, C.c_int32, C.c_int32, _p, _p, _p, C.c_size_t]),
    "jpeg_amd_project_batch": (C.c_int, [_p, C.c_int, _p, C.c_size_t, _p, _p, _p, C.c_int32, C.c_int32, _p, C.c_size_t]),
    "jpeg_amd_project_tensor_batch": (C.c_int, [_p, C.c_int, _p, C.c_size_t, _p, _p, _p, C.c_int32, C.c_int32, _p, _p, _p, _p,
                                                C.c_size_t]),
    "jpeg_amd_project_view": (C.c_int, [_L, C.c_int, _p, C.c_int32, C.c_int32, _p, _p]),
    "jpeg_amd_decode_projected_mixed": (C.c_int, [_p, C.c_int, _p, C.c_int, C.c_int, _p, _p, _p, C.c_int32, C.c_int32, _p, _p, _p,
                                                  C.c_size_t]),
    "jpeg_amd_decode_tensor_projected_mixed": (C.c_int, [_p, C.c_int, _p, C.c_int, C.c_int, _p, _p, _p, C.c_int32, C.c_int32, _p, _p,
                                                         _p, _p, _p, _p, C.c_size_t]),
    "jpeg_amd_decompress_resized_projected_mixed": (C.c_int, [_p, _pp, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _p, C.c_int32,
                                                              C.c_int32, _p, C.c_size_t, _p, _p, _p, _p]),
    "jpeg_amd_decompress_tensor_projected_mixed": (C.c_int, [_p, _pp, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _p, C.c_int32,
                                                             C.c_int32, _p, _p, _p, _p, C.c_size_t, _p, _p, _p, _p]),
    # "bicubic warp": the projective calls with `int filter` behind the warp (the view: behind the matrix)
    "jpeg_amd_project_filter_batch": (C.c_int, [_p, C.c_int, _p, C.c_size_t, _p, _p, _p, C.c_int, C.c_int32, C.c_int32, _p, C.c_size_t]),
    "jpeg_amd_project_filter_tensor_batch": (C.c_int, [_p, C.c_int, _p, C.c_size_t, _p, _p, _p, C.c_int, C.c_int32, C.c_int32, _p, _p,
                                                       _p, _p, C.c_size_t]),
    "jpeg_amd_project_filter_view": (C.c_int, [_L, C.c_int, _p, C.c_int, C.c_int32, C.c_int32, _p, _p]),
    "jpeg_amd_decode_projected_filter_mixed": (C.c_int, [_p, C.c_int, _p, C.c_int, C.c_int, _p, _p, _p, C.c_int, C.c_int32, C.c_int32,
                                                         _p, _p, _p, C.c_size_t]),
    "jpeg_amd_decode_tensor_projected_filter_mixed": (C.c_int, [_p, C.c_int, _p, C.c_int, C.c_int, _p, _p, _p, C.c_int, C.c_int32,
                                                                C.c_int32, _p, _p, _p, _p, _p, _p, C.c_size_t]),
    "jpeg_amd_decompress_resized_projected_filter_mixed": (C.c_int, [_p, _pp, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _p, C.c_int,
                                                                     C.c_int32, C.c_int32, _p, C.c_size_t, _p, _p, _p, _p]),
    "jpeg_amd_decompress_tensor_projected_filter_mixed": (C.c_int, [_p, _pp, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _p, C.c_int,
                                                                    C.c_int32, C.c_int32, _p, _p, _p, _p, C.c_size_t, _p, _p, _p, _p]),
    "jpeg_amd_warp_view": (C.c_int, [_L, C.c_int, _p, C.c_int32, C.c_int32, _p, _p]),
    "jpeg_amd_decode_warped_mixed": (C.c_int, [_p, C.c_int, _p, C.c_int, C.c_int, _p, _p, _p, C.c_int32, C.c_int32, _p, _p, _p,
                                               C.c_size_t]),
    "jpeg_amd_decode_tensor_warped_mixed": (C.c_int, [_p, C.c_int, _p, C.c_int, C.c_int, _p, _p, _p, C.c_int32, C.c_int32, _p, _p, _p,
                                                      _p, _p, C.c_size_t]),
    "jpeg_amd_decompress_resized_warped_mixed": (C.c_int, [_p, _pp, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _p, C.c_int32,
                                                           C.c_int32, _p, C.c_size_t, _p, _p, _p, _p]),
    "jpeg_amd_decompress_tensor_warped_mixed": (C.c_int, [_p, _pp, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _p, C.c_int32,
                                                          C.c_int32, _p, _p, _p, C.c_size_t, _p, _p, _p, _p]),
    # "colour stage": the arguments of the call each is named after, and the colour in front of the output pointer
    "jpeg_amd_resize_colour_tensor_batch": (C.c_int, [_p, C.c_int, _p, C.c_size_t, _p, C.c_int32, C.c_int32, C.c_int, _p, _p, _p, _p,
                                                      _p, _p, _p, C.c_size_t]),
    "jpeg_amd_decode_tensor_colour_mixed": (C.c_int, [_p, C.c_int, _p, C.c_int, C.c_int, _p, C.c_int32, C.c_int32, C.c_int, _p, _p,
                                                      _p, _p, _p, _p, _p, C.c_size_t]),
    "jpeg_amd_decompress_tensor_colour_mixed": (C.c_int, [_p, _pp, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, C.c_int32, C.c_int32,
                                                          C.c_int, _p, _p, _p, _p, _p, _p, _p, C.c_size_t, _p, _p, _p]),
    "jpeg_amd_warp_colour_tensor_batch": (C.c_int, [_p, C.c_int, _p, C.c_size_t, _p, _p, _p, C.c_int32, C.c_int32, _p, _p, _p, _p,
                                                    C.c_size_t]),
    "jpeg_amd_decode_tensor_warped_colour_mixed": (C.c_int, [_p, C.c_int, _p, C.c_int, C.c_int, _p, _p, _p, C.c_int32, C.c_int32, _p,
                                                             _p, _p, _p, _p, _p, C.c_size_t]),
    "jpeg_amd_decompress_tensor_warped_colour_mixed": (C.c_int, [_p, _pp, _p, C.c_int, C.c_int, C.c_int, C.c_int, _p, _p, _p, C.c_int32,
                                                                 C.c_int32, _p, _p, _p, _p, C.c_size_t, _p, _p, _p, _p]),
}


class Region(C.Structure):
    """struct jpeg_amd_region"""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


class Placement(C.Structure):
    """struct jpeg_amd_placement"""
    _fields_ = [("mode", C.c_int32), ("anchor", C.c_int32), ("h_windows", C.c_void_p), ("fill", C.c_uint8 * 3),
                ("reserved", C.c_uint8)]


class Warp(C.Structure):
    """struct jpeg_amd_warp"""
    _fields_ = [("edge", C.c_int32), ("fill", C.c_uint8 * 3)]


class Colour(C.Structure):
    """struct jpeg_amd_colour"""
    _fields_ = [("h_matrices", C.c_void_p), ("lo", C.c_float), ("hi", C.c_float)]


class View(C.Structure):
    """struct jpeg_amd_view"""
    _fields_ = [("denom", C.c_int32), ("region", Region)]


class Image(C.Structure):
    """struct jpeg_amd_image"""
    _fields_ = [("layout", Layout), ("d_coef", C.c_void_p * MAX_PLANES), ("d_quanta", C.c_void_p), ("ntables", C.c_int32)]


class ExpandItem(C.Structure):
    """struct jpeg_amd_expand_item"""
    _fields_ = [("layout", Layout), ("d_coef", C.c_void_p * MAX_PLANES), ("window", Region * MAX_PLANES), ("head", C.c_int32),
                ("desc_at", C.c_uint64), ("entries_at", C.c_uint64)]


class Extent(C.Structure):
    """struct jpeg_amd_extent"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32)]


class TensorSpec(C.Structure):
    """struct jpeg_amd_tensor_spec"""
    _fields_ = [("dtype", C.c_int32), ("layout", C.c_int32), ("mean", C.c_float * 3), ("scale", C.c_float * 3)]


class TensorSource(C.Structure):
    """struct jpeg_amd_tensor_source"""
    _fields_ = [("dtype", C.c_int32), ("layout", C.c_int32), ("scale", C.c_float * 3), ("offset", C.c_float * 3)]


F32, F16, BF16 = 0, 1, 2                # JPEG_AMD_F32 ...
U8 = 3                                  # JPEG_AMD_U8: tensor sources only
TENSOR_HWC, TENSOR_CHW = 0, 1           # JPEG_AMD_TENSOR_HWC ...
FILTER_BILINEAR, FILTER_ANTIALIAS = 0, 1  # JPEG_AMD_FILTER_BILINEAR ...
FILTER_BICUBIC = 3                        # JPEG_AMD_FILTER_BICUBIC (2 is no filter)
PLACE_WINDOWS, PLACE_FIT, PLACE_FIT_DOWN = 0, 1, 2   # JPEG_AMD_PLACE_*
ANCHOR_CENTRE, ANCHOR_TOP_LEFT = 0, 1               # JPEG_AMD_ANCHOR_*
EDGE_FILL, EDGE_REPLICATE = 0, 1                    # JPEG_AMD_EDGE_*
ORIENT_EXIF = 0                       # JPEG_AMD_ORIENT_EXIF (the file calls); JPEG_AMD_ORIENT_1 .. _8 are 1 .. 8

# JPEG_AMD_XFORM_*: TRANSPOSE, then FLIP_H, then FLIP_V
XFORM_TRANSPOSE, XFORM_FLIP_H, XFORM_FLIP_V = 1, 2, 4
XFORM = {"none": 0, "transpose": 1, "flip_h": 2, "flip_v": 4, "rot_180": 6, "rot_ccw": 5, "rot_cw": 3, "transverse": 7,
         "ii": 5, "iii": 6, "iv": 3}


class FrameInfo(C.Structure):
    """struct jpeg_amd_frame_info"""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("precision", C.c_int32), ("ncomponents", C.c_int32),
        ("process", C.c_int32), ("scale_x", C.c_int32), ("scale_y", C.c_int32),
        ("id", C.c_int32 * MAX_PLANES), ("factor_x", C.c_int32 * MAX_PLANES), ("factor_y", C.c_int32 * MAX_PLANES),
        ("units_x", C.c_int32 * MAX_PLANES), ("units_y", C.c_int32 * MAX_PLANES),
        ("nscans", C.c_int32), ("restart_interval", C.c_int32),
    ]


class Scan(C.Structure):
    """struct jpeg_amd_scan"""
    _fields_ = [("ncomponents", C.c_int32), ("component", C.c_int32 * MAX_PLANES),
                ("dc", C.c_int32 * MAX_PLANES), ("ac", C.c_int32 * MAX_PLANES),
                ("band_lo", C.c_int32), ("band_hi", C.c_int32), ("bit", C.c_int32), ("refine", C.c_int32)]


class Jfif(C.Structure):
    """struct jpeg_amd_jfif"""
    _fields_ = [("version_minor", C.c_int32), ("unit", C.c_int32), ("density_x", C.c_int32), ("density_y", C.c_int32)]


class Metadata(C.Structure):
    """struct jpeg_amd_metadata"""
    _fields_ = [("kind", C.c_int32), ("app", C.c_int32), ("jfif", Jfif), ("data", C.c_void_p), ("size", C.c_size_t)]


_LIB = None


def lib() -> C.CDLL:
    """Load libjpeg_amd.so (built by jpeg_amd.build / __graft_entry__.build())."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: run `python -m jpeg_amd.build` (hipcc, gfx950). "
                "jpeg_amd has no CPU fallback.")
        # PyTorch-ROCm ships its own HIP runtime; when both live in one process it has to be the
        # one loaded FIRST, otherwise the context created later sees no device (ENODEV).  The
        # host-only entry points (entropy coder) do not need torch at all: a missing torch is fine.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the header and the library diverge
            fn.restype, fn.argtypes = res, args
        _LIB = L
    return _LIB


def check(status: int, what: str, ctx=None) -> None:
    if status != OK:
        hip = lib().jpeg_amd_last_hip_error(ctx) if ctx else 0
        raise JpegAmdError(status, what, hip)


def ptr_array(ptrs):
    arr = (C.c_void_p * MAX_PLANES)()
    for i, p in enumerate(ptrs):
        arr[i] = p
    return arr


def size_array(vals):
    arr = (C.c_size_t * MAX_PLANES)()
    for i, v in enumerate(vals):
        arr[i] = v
    return arr
