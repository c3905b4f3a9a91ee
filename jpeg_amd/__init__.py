"""jpeg_amd -- MI355X-native (gfx950) spectral pipeline of tayloraswift/jpeg.

Host-side mirror of the reference's types for the hot path (Spectral / Planar /
Rectangular, JPEG.Layout, the YCbCr / RGB colour targets) over the C ABI in
include/jpeg_amd.h.  All arithmetic runs in hand-written HIP kernels
(jpeg_amd/csrc); there is no CPU fallback -- a missing library raises.
"""
from ._lib import JpegAmdError, LIB_PATH  # noqa: F401
from .api import (  # noqa: F401
    RGB, YCbCr, Component, Context, Layout, Planar, Rectangular, Scan, Spectral,
    compress_tensors, compression_quanta, decode_crops_resized, decode_crops_tensor, decode_crops_tensor_mixed, decode_regions, decode_resized,
    decode_resized_mixed, decode_scaled, decode_tensors, decode_tensors_mixed, decode_views, decode_views_mixed, decompress_resized, decompress_tensors,
    default_context,
    encode_tensors, exif_orientation, inspect, orient_region, place_window, reduce, reduce_layout, region_window, resize, resize_tensor, scaled_size, tensor_pixels, tensor_source, tensor_spec,
    transform, transform_quanta, view_denom, view_of_source, view_window,
    affine_matrix, decode_tensors_warped_mixed, decode_warped_mixed, warp, warp_tensor, warp_view,
    colour_matrix,
    decompress_spectrals, plan_intervals,
    decode_projected_mixed, decode_tensors_projected_mixed, perspective_matrix, project, project_tensor, project_view,
)

__all__ = ["RGB", "YCbCr", "Component", "Context", "Layout", "Planar", "Rectangular",
           "Scan", "Spectral", "JpegAmdError", "compress_tensors", "compression_quanta", "decode_crops_resized", "decode_crops_tensor", "decode_crops_tensor_mixed",
           "decode_regions", "decode_resized", "decode_resized_mixed", "decode_scaled", "decode_tensors", "decode_tensors_mixed",
           "decode_views", "decode_views_mixed", "decompress_resized", "decompress_tensors", "default_context", "encode_tensors", "exif_orientation", "inspect", "orient_region", "place_window", "reduce", "reduce_layout",
           "region_window", "resize", "resize_tensor", "scaled_size", "tensor_pixels", "tensor_source", "tensor_spec", "transform", "transform_quanta", "view_denom",
           "view_of_source", "view_window", "affine_matrix", "decode_tensors_warped_mixed", "decode_warped_mixed", "warp", "warp_tensor",
           "warp_view", "colour_matrix", "decode_projected_mixed", "decode_tensors_projected_mixed", "perspective_matrix", "project",
           "project_tensor", "project_view", "decompress_spectrals", "plan_intervals"]
