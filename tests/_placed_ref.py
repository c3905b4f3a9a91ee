"""The placed resample of include/jpeg_amd.h ("placed resample") restated in numpy and Python integers: the canvas with an
image in a window and the fill around it, and the window of the FIT modes.  The contract is by reference -- inside the window
the filter's existing contract at the window's size -- so `place` takes an image that one of the existing mirrors
(_resize_ref, _antialias_ref, _bicubic_ref) has already resampled to ww x wh.  Independent of the code under test; importing
this needs no GPU and no torch."""
import numpy as np

WINDOWS, FIT, FIT_DOWN = 0, 1, 2          # JPEG_AMD_PLACE_*
CENTRE, TOP_LEFT = 0, 1                   # JPEG_AMD_ANCHOR_*


def place(resized, window, canvas, fill):
    """resized: uint8 [wh, ww, 3], the filter's output at the window's size; window (x0, y0, ww, wh); canvas (out_w, out_h);
    fill: three bytes -> uint8 [out_h, out_w, 3].  (A flip mirrors this whole canvas afterwards: _tensor_ref.normalise.)"""
    x0, y0, ww, wh = (int(v) for v in window)
    out_w, out_h = canvas
    resized = np.asarray(resized)
    assert resized.dtype == np.uint8 and resized.shape == (wh, ww, 3)
    assert ww >= 1 and wh >= 1 and 0 <= x0 <= out_w - ww and 0 <= y0 <= out_h - wh
    out = np.empty((out_h, out_w, 3), np.uint8)
    out[:, :] = np.asarray(fill, np.uint8)
    out[y0:y0 + wh, x0:x0 + ww] = resized
    return out


def place_window(mode, anchor, src_w, src_h, out_w, out_h):
    """The header's integers (Python's are unbounded: no overflow to think about) -> (x0, y0, ww, wh)."""
    assert mode in (FIT, FIT_DOWN) and anchor in (CENTRE, TOP_LEFT)
    assert src_w >= 1 and src_h >= 1 and out_w >= 1 and out_h >= 1
    if mode == FIT_DOWN and src_w <= out_w and src_h <= out_h:
        ww, wh = src_w, src_h
    elif out_w * src_h <= out_h * src_w:                       # the width binds
        ww, wh = out_w, min(out_h, max(1, (2 * src_h * out_w + src_w) // (2 * src_w)))
    else:
        ww, wh = min(out_w, max(1, (2 * src_w * out_h + src_h) // (2 * src_h))), out_h
    if anchor == CENTRE:
        return ((out_w - ww) // 2, (out_h - wh) // 2, ww, wh)
    return (0, 0, ww, wh)
