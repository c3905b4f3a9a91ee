"""Which library call a public resample function makes, and with which arguments -- no GPU.  A recorder stands in for the
library (pytest's monkeypatch on _lib.lib): it notes the symbol and its arguments and answers 0; a stand-in context hands out
host tensors.  Every public resample function is called with every subset of its optional columns (orientations, placement,
colour, flips, a warp of 6 or of 9 numbers, source rectangles), and of each call the test asserts that the ONE symbol called is
the widest entry point of its cell (source x byte or tensor target x map), that every host argument has the right bytes, that
a column the call does not carry is NULL, and that the output pointer and stride are those of the tensor that comes back.

The expected arguments are not reasoned out: tests/golden/resample_routes.json holds what the public functions passed when
each still chose the narrowest symbol that could carry its arguments (this module run as a program records it).  WIDE and ARGS,
below, map such a narrow call onto its wide form as the delegations in csrc/capi_view.hip and csrc/capi_files.hip do: the same
arguments by name, NULL for what the narrow form lacks.  They are the only hand-written part.  The record also holds a handful
of doubly wrong calls with the ValueError each raised, which pins the order of the Python-side checks."""
import ctypes as C
import functools
import hashlib
import itertools
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import jpeg_amd as J
from _files import synthetic_file
from jpeg_amd import _lib, api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_routes.json")

# ---- the hand-written part: the arguments of every symbol by name, and the wide form of every narrow one ------------------------
IMAGES = "ctx n src src_stride extents "
BATCH = "ctx layout n planes plane_strides quanta quanta_stride ntables cosited color views "
MIXED = "ctx n images cosited color "
FILES = "ctx files sizes n threads cosited color "
CANVAS, MAP, TENSOR, COLUMNS, DST = "wt ht code ", "matrices warp wt ht ", "spec flips ", "orient place windows_out ", "out stride "
INFO = "infos views_out "
ARGS = {name: args.split() for name, args in {
    "jpeg_amd_resize_filter_batch": IMAGES + CANVAS + DST,
    "jpeg_amd_resize_oriented_batch": IMAGES + CANVAS + "orient " + DST,
    "jpeg_amd_resize_placed_batch": IMAGES + CANVAS + COLUMNS + DST,
    "jpeg_amd_resize_filter_tensor_batch": IMAGES + CANVAS + TENSOR + DST,
    "jpeg_amd_resize_oriented_tensor_batch": IMAGES + CANVAS + TENSOR + "orient " + DST,
    "jpeg_amd_resize_placed_tensor_batch": IMAGES + CANVAS + TENSOR + COLUMNS + DST,
    "jpeg_amd_resize_colour_tensor_batch": IMAGES + CANVAS + TENSOR + COLUMNS + "colour " + DST,
    "jpeg_amd_warp_batch": IMAGES + MAP + DST,
    "jpeg_amd_warp_tensor_batch": IMAGES + MAP + TENSOR + DST,
    "jpeg_amd_warp_colour_tensor_batch": IMAGES + MAP + TENSOR + "colour " + DST,
    "jpeg_amd_project_batch": IMAGES + MAP + DST,
    "jpeg_amd_project_tensor_batch": IMAGES + MAP + TENSOR + "colour " + DST,
    "jpeg_amd_decode_resized_filter_batch": BATCH + CANVAS + DST,
    "jpeg_amd_decode_tensor_filter_batch": BATCH + CANVAS + TENSOR + DST,
    "jpeg_amd_decode_resized_filter_mixed": MIXED + "views " + CANVAS + DST,
    "jpeg_amd_decode_resized_oriented_mixed": MIXED + "views " + CANVAS + "orient " + DST,
    "jpeg_amd_decode_resized_placed_mixed": MIXED + "views " + CANVAS + COLUMNS + DST,
    "jpeg_amd_decode_tensor_filter_mixed": MIXED + "views " + CANVAS + TENSOR + DST,
    "jpeg_amd_decode_tensor_oriented_mixed": MIXED + "views " + CANVAS + TENSOR + "orient " + DST,
    "jpeg_amd_decode_tensor_placed_mixed": MIXED + "views " + CANVAS + TENSOR + COLUMNS + DST,
    "jpeg_amd_decode_tensor_colour_mixed": MIXED + "views " + CANVAS + TENSOR + COLUMNS + "colour " + DST,
    "jpeg_amd_decode_warped_mixed": MIXED + "orient " + MAP + "views_out matrices_out " + DST,
    "jpeg_amd_decode_tensor_warped_mixed": MIXED + "orient " + MAP + TENSOR + "views_out matrices_out " + DST,
    "jpeg_amd_decode_tensor_warped_colour_mixed": MIXED + "orient " + MAP + TENSOR + "views_out matrices_out colour " + DST,
    "jpeg_amd_decode_projected_mixed": MIXED + "orient " + MAP + "views_out matrices_out " + DST,
    "jpeg_amd_decode_tensor_projected_mixed": MIXED + "orient " + MAP + TENSOR + "views_out matrices_out colour " + DST,
    "jpeg_amd_decompress_resized_mixed": FILES + "regions " + CANVAS + DST + INFO,
    "jpeg_amd_decompress_resized_oriented_mixed": FILES + "regions " + CANVAS + "orient " + DST + INFO + "orient_out",
    "jpeg_amd_decompress_resized_placed_mixed": FILES + "regions " + CANVAS + COLUMNS + DST + INFO + "orient_out",
    "jpeg_amd_decompress_tensor_mixed": FILES + "regions " + CANVAS + TENSOR + DST + INFO,
    "jpeg_amd_decompress_tensor_oriented_mixed": FILES + "regions " + CANVAS + TENSOR + "orient " + DST + INFO + "orient_out",
    "jpeg_amd_decompress_tensor_placed_mixed": FILES + "regions " + CANVAS + TENSOR + COLUMNS + DST + INFO + "orient_out",
    "jpeg_amd_decompress_tensor_colour_mixed": FILES + "regions " + CANVAS + TENSOR + COLUMNS + "colour " + DST + INFO + "orient_out",
    "jpeg_amd_decompress_resized_warped_mixed": FILES + "orient " + MAP + DST + INFO + "matrices_out orient_out",
    "jpeg_amd_decompress_tensor_warped_mixed": FILES + "orient " + MAP + TENSOR + DST + INFO + "matrices_out orient_out",
    "jpeg_amd_decompress_tensor_warped_colour_mixed": FILES + "orient " + MAP + TENSOR + "colour " + DST + INFO + "matrices_out orient_out",
    "jpeg_amd_decompress_resized_projected_mixed": FILES + "orient " + MAP + DST + INFO + "matrices_out orient_out",
    "jpeg_amd_decompress_tensor_projected_mixed": FILES + "orient " + MAP + TENSOR + "colour " + DST + INFO + "matrices_out orient_out",
}.items()}
# narrow -> the widest entry point of its cell; a symbol that is not a key is the widest of its cell
WIDE = {
    "jpeg_amd_resize_filter_batch": "jpeg_amd_resize_placed_batch",
    "jpeg_amd_resize_oriented_batch": "jpeg_amd_resize_placed_batch",
    "jpeg_amd_resize_filter_tensor_batch": "jpeg_amd_resize_colour_tensor_batch",
    "jpeg_amd_resize_oriented_tensor_batch": "jpeg_amd_resize_colour_tensor_batch",
    "jpeg_amd_resize_placed_tensor_batch": "jpeg_amd_resize_colour_tensor_batch",
    "jpeg_amd_warp_tensor_batch": "jpeg_amd_warp_colour_tensor_batch",
    "jpeg_amd_decode_resized_filter_mixed": "jpeg_amd_decode_resized_placed_mixed",
    "jpeg_amd_decode_resized_oriented_mixed": "jpeg_amd_decode_resized_placed_mixed",
    "jpeg_amd_decode_tensor_filter_mixed": "jpeg_amd_decode_tensor_colour_mixed",
    "jpeg_amd_decode_tensor_oriented_mixed": "jpeg_amd_decode_tensor_colour_mixed",
    "jpeg_amd_decode_tensor_placed_mixed": "jpeg_amd_decode_tensor_colour_mixed",
    "jpeg_amd_decode_tensor_warped_mixed": "jpeg_amd_decode_tensor_warped_colour_mixed",
    "jpeg_amd_decompress_resized_mixed": "jpeg_amd_decompress_resized_placed_mixed",
    "jpeg_amd_decompress_resized_oriented_mixed": "jpeg_amd_decompress_resized_placed_mixed",
    "jpeg_amd_decompress_tensor_mixed": "jpeg_amd_decompress_tensor_colour_mixed",
    "jpeg_amd_decompress_tensor_oriented_mixed": "jpeg_amd_decompress_tensor_colour_mixed",
    "jpeg_amd_decompress_tensor_placed_mixed": "jpeg_amd_decompress_tensor_colour_mixed",
    "jpeg_amd_decompress_tensor_warped_mixed": "jpeg_amd_decompress_tensor_warped_colour_mixed",
}
# The cells: every symbol a public resample function may reach.
CELLS = {
    "jpeg_amd_resize_placed_batch", "jpeg_amd_resize_colour_tensor_batch", "jpeg_amd_warp_batch", "jpeg_amd_warp_colour_tensor_batch",
    "jpeg_amd_project_batch", "jpeg_amd_project_tensor_batch", "jpeg_amd_decode_resized_filter_batch",
    "jpeg_amd_decode_tensor_filter_batch", "jpeg_amd_decode_resized_placed_mixed", "jpeg_amd_decode_tensor_colour_mixed",
    "jpeg_amd_decode_warped_mixed", "jpeg_amd_decode_tensor_warped_colour_mixed", "jpeg_amd_decode_projected_mixed",
    "jpeg_amd_decode_tensor_projected_mixed", "jpeg_amd_decompress_resized_placed_mixed", "jpeg_amd_decompress_tensor_colour_mixed",
    "jpeg_amd_decompress_resized_warped_mixed", "jpeg_amd_decompress_tensor_warped_colour_mixed",
    "jpeg_amd_decompress_resized_projected_mixed", "jpeg_amd_decompress_tensor_projected_mixed",
}


def widen(symbol, args):
    """A recorded call as the widest entry point of its cell receives it: NULL for what the recorded form lacks.  The room for
    the orientations applied is there in every wide file call, whether the recorded call gave one or not."""
    wide = WIDE.get(symbol, symbol)
    out = {name: args.get(name) for name in ARGS[wide]}
    if "orient_out" in out:
        out["orient_out"] = ["room", args["n"]]
    return wide, out


# ---- the recorder ---------------------------------------------------------------------------------------------------------------

def _floats(ptr, count):
    return C.string_at(ptr, 4 * count).hex()


def _regions(arr, n):
    return [[r.x, r.y, r.width, r.height] for r in arr[:n]]


def describe(symbol, values):
    """The arguments of one call by name, as JSON holds them: numbers as they are, host arrays and structures by their
    contents, floats as the hex of their bytes, files and what a tensor's pointer points at by their SHA-256, room for results
    as its length.  `raw` holds the two pointers that the results are compared with."""
    a = dict(zip(ARGS[symbol], values))
    assert len(values) == len(ARGS[symbol]), symbol
    n = max(a["n"], 0)
    k = 9 if "project" in symbol else 6
    d, raw = {}, {}
    digest = lambda ptr, nbytes: hashlib.sha256(C.string_at(ptr, nbytes)).hexdigest()   # noqa: E731
    for name, v in a.items():
        if name == "out":
            raw[name], d[name] = v, "the tensor that comes back"
        elif name == "src":
            d[name] = digest(v, n * a["src_stride"])
        elif name == "quanta":
            d[name] = digest(v, 2 * n * a["quanta_stride"])
        elif name == "planes":
            d[name] = [digest(v[p], 2 * n * a["plane_strides"][p]) for p in range(a["layout"]._obj.nplanes)]
        elif name == "ctx":
            d[name] = v.value
        elif v is None or isinstance(v, int):
            d[name] = v
        elif name == "extents":
            d[name] = [[e.width, e.height] for e in v[:n]]
        elif name in ("views", "views_out"):
            d[name] = [[t.denom, t.region.x, t.region.y, t.region.width, t.region.height] for t in v[:n]]
        elif name in ("orient", "flips", "sizes", "plane_strides"):
            d[name] = list(v[:n] if name != "plane_strides" else v[:])
        elif name in ("regions", "windows_out"):
            d[name] = _regions(v, n)
        elif name in ("spec", "warp", "layout"):
            d[name] = bytes(v._obj).hex()
        elif name == "place":
            p = v._obj
            d[name] = {"mode": p.mode, "anchor": p.anchor, "fill": list(p.fill), "reserved": p.reserved,
                       "windows": _regions(C.cast(p.h_windows, C.POINTER(_lib.Region)), n) if p.h_windows else None}
        elif name == "colour":
            d[name] = {"clamp": bytes(v._obj)[8:16].hex(), "matrices": _floats(v._obj.h_matrices, 12 * n)}
        elif name == "files":
            d[name] = [digest(v[i], a["sizes"][i]) for i in range(n)]
        elif name == "images":
            d[name] = [{"layout": bytes(im.layout).hex(), "ntables": im.ntables, "quanta": digest(im.d_quanta, 128 * im.ntables),
                        "planes": [digest(im.d_coef[p], 128 * im.layout.units_x[p] * im.layout.units_y[p]) for p in range(im.layout.nplanes)]}
                       for im in v[:n]]
        elif name == "infos":
            d[name] = ["room", len(v)] if isinstance(v, C.Array) and v._type_ is _lib.FrameInfo else "?"
        elif name == "orient_out":
            d[name] = ["room", len(v)] if isinstance(v, C.Array) and v._type_ is C.c_int32 else "?"
        else:
            raise AssertionError(name)
    if "matrices" in a:
        d["matrices"] = _floats(a["matrices"], k * n)
    if "matrices_out" in a:
        raw["matrices_out"], d["matrices_out"] = a["matrices_out"], ["room", k * n]
    return d, raw


class Recorder:
    """In the place of the library: the resample entry points are noted and answer 0; every other symbol (the geometry helpers
    that the crop functions ask on the host) is the library's own."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name in ARGS:
            return functools.partial(self.note, name)
        return getattr(self.real, name)

    def note(self, name, *values):
        self.calls.append((name,) + describe(name, values))      # (now: what the pointers point at lives as long as the call)
        return 0


class StandIn:
    """A context without a device: a handle, host tensors (zeroed: the packed images have gaps), uploads that stay on the host."""
    handle = C.c_void_p(0x5A5A)

    def empty(self, n, dtype):
        return torch.zeros(max(int(n), 0), dtype=dtype)

    def upload(self, a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


# ---- the inputs: two of everything, of different sizes ----------------------------------------------------------------------------
N = 2
OUT = (10, 6)
CTX = StandIn()
SPEC = functools.lru_cache(maxsize=None)(lambda: J.tensor_spec(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), layout="chw"))
FILTERS = ("bilinear", "antialias", "bicubic")
M6 = np.array([[1.5, 0.25, 1.0, -0.125, 1.25, 0.5], [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]], np.float32)
M9 = np.concatenate([M6, np.array([[0.001, 0.002, 1.0], [0.0, 0.0, 1.0]], np.float32)], axis=1)
COLUMNS_OF = {                                         # column -> the values it takes, the first one "absent"
    "orient": (None, [6, 1]),
    "place": (None, "fit", [(1, 1, 8, 4), (0, 0, 10, 6)]),
    "colour": (None, True),
    "flips": (None, [1, 0]),
    "regions": (None, [(2, 2, 16, 12), (0, 0, 16, 16)]),
    "exif": (None, "exif", [6, "exif"]),
    "map": (6, 9),
}


@functools.lru_cache(maxsize=None)
def files():
    return [synthetic_file("420", (24, 16), 3)[0], synthetic_file("444", (16, 16), 4)[0]]


def pictures():
    rng = np.random.default_rng(5)
    return [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in ((7, 5), (4, 9))]


def spectrals():
    out = []
    for seed, (size, factors) in enumerate((((24, 16), [(2, 2), (1, 1), (1, 1)]), ((16, 16), [(1, 1)] * 3))):
        layout = J.Layout("ycc8", {c + 1: J.Component(f, min(c, 1)) for c, f in enumerate(factors)})
        rng = np.random.default_rng(seed)
        planes = [rng.integers(-64, 64, (uy, ux, 64)).astype(np.int16) for ux, uy in layout.units(size)]
        quanta = [rng.integers(1, 24, 64).astype(np.uint16) for _ in range(2)]
        out.append(J.Spectral.from_host(CTX, size, layout, planes, quanta))
    return out


def batch():
    layout = J.Layout("ycc8", {1: J.Component((2, 2), 0), 2: J.Component((1, 1), 1), 3: J.Component((1, 1), 1)})
    rng = np.random.default_rng(9)
    planes = [torch.from_numpy(rng.integers(-64, 64, (N, uy, ux, 64)).astype(np.int16)) for ux, uy in layout.units((24, 16))]
    quanta = rng.integers(1, 24, (N, 2, 64)).astype(np.uint16)
    return (24, 16), layout, planes, quanta


VIEWS = [(1, 2, 1, 20, 12), (2, 0, 0, 8, 8)]
CROPS = [(2, 2, 16, 12), (0, 0, 16, 16)]


def keywords(case, names):
    """The keyword arguments of a case for the columns `names` that its function has."""
    kw = {}
    if "orient" in names and case.get("orient") is not None:
        kw["orientations"] = case["orient"]
    if "exif" in names and case.get("exif") is not None:
        kw["orientation"] = case["exif"]
    if "place" in names and case.get("place") is not None:
        kw.update(place=case["place"], anchor="top-left", fill=(7, 8, 9))
    if "colour" in names and case.get("colour"):
        kw.update(colour=[J.colour_matrix(brightness=1.25, hue=0.1), J.colour_matrix(grey=True)], colour_clamp=(0.0, 255.0))
    if "flips" in names and case.get("flips") is not None:
        kw["flips"] = case["flips"]
    if "regions" in names and case.get("regions") is not None:
        kw["source_regions"] = case["regions"]
    return kw


def mapped_keywords(case, names):
    kw = keywords(case, names)
    kw.update(edge="replicate", fill=(3, 4, 5))
    return kw


# function -> (its columns, how a case calls it).  `f`: a filter, taken in turn from FILTERS.
FUNCTIONS = {
    "resize": ("orient place", lambda c, f: api.resize(CTX, pictures(), OUT, filter=f, **keywords(c, "orient place"))),
    "resize_tensor": ("orient place colour flips",
                      lambda c, f: api.resize_tensor(CTX, pictures(), OUT, SPEC(), filter=f, **keywords(c, "orient place colour flips"))),
    "warp": ("", lambda c, f: api.warp(CTX, pictures(), M6, OUT, **mapped_keywords(c, ""))),
    "warp_tensor": ("colour flips", lambda c, f: api.warp_tensor(CTX, pictures(), M6, OUT, SPEC(), **mapped_keywords(c, "colour flips"))),
    "project": ("", lambda c, f: api.project(CTX, pictures(), M9.reshape(N, 3, 3), OUT, **mapped_keywords(c, ""))),
    "project_tensor": ("colour flips", lambda c, f: api.project_tensor(CTX, pictures(), M9, OUT, SPEC(), **mapped_keywords(c, "colour flips"))),
    "decode_resized": ("", lambda c, f: api.decode_resized(CTX, *batch(), VIEWS, OUT, cosite=True, filter=f)),
    "decode_tensors": ("flips", lambda c, f: api.decode_tensors(CTX, *batch(), VIEWS, OUT, SPEC(), color=J.YCbCr, filter=f,
                                                                 **keywords(c, "flips"))),
    "decode_crops_resized": ("", lambda c, f: api.decode_crops_resized(CTX, *batch(), CROPS, OUT, filter=f)),
    "decode_crops_tensor": ("flips", lambda c, f: api.decode_crops_tensor(CTX, *batch(), CROPS, OUT, SPEC(), filter=f, **keywords(c, "flips"))),
    "decode_resized_mixed": ("orient place", lambda c, f: api.decode_resized_mixed(CTX, spectrals(), VIEWS, OUT, cosite=True, filter=f,
                                                                                     **keywords(c, "orient place"))),
    "decode_tensors_mixed": ("orient place colour flips",
                             lambda c, f: api.decode_tensors_mixed(CTX, spectrals(), VIEWS, OUT, SPEC(), color=J.YCbCr, filter=f,
                                                                   **keywords(c, "orient place colour flips"))),
    "decode_crops_tensor_mixed": ("orient place colour flips",
                                  lambda c, f: api.decode_crops_tensor_mixed(CTX, spectrals(), [(2, 2, 12, 12), (0, 0, 16, 16)], OUT, SPEC(),
                                                                             filter=f, **keywords(c, "orient place colour flips"))),
    "decode_warped_mixed": ("orient", lambda c, f: api.decode_warped_mixed(CTX, spectrals(), M6, OUT, **mapped_keywords(c, "orient"))),
    "decode_tensors_warped_mixed": ("orient colour flips",
                                    lambda c, f: api.decode_tensors_warped_mixed(CTX, spectrals(), M6, OUT, SPEC(), cosite=True,
                                                                                 **mapped_keywords(c, "orient colour flips"))),
    "decode_projected_mixed": ("orient", lambda c, f: api.decode_projected_mixed(CTX, spectrals(), M9, OUT, **mapped_keywords(c, "orient"))),
    "decode_tensors_projected_mixed": ("orient colour flips",
                                       lambda c, f: api.decode_tensors_projected_mixed(CTX, spectrals(), M9.reshape(N, 3, 3), OUT, SPEC(),
                                                                                       color=J.YCbCr, **mapped_keywords(c, "orient colour flips"))),
    "decompress_tensors": ("regions exif place colour flips",
                           lambda c, f: api.decompress_tensors(CTX, files(), OUT, SPEC(), filter=f, threads=3,
                                                               **keywords(c, "regions exif place colour flips"))),
    "decompress_resized": ("regions exif place",
                           lambda c, f: api.decompress_resized(CTX, files(), OUT, filter=f, cosite=True, **keywords(c, "regions exif place"))),
    "decompress_tensors(warp)": ("map exif colour flips",
                                 lambda c, f: api.decompress_tensors(CTX, files(), OUT, SPEC(), warp=M9 if c["map"] == 9 else M6,
                                                                     **mapped_keywords(c, "exif colour flips"))),
    "decompress_resized(warp)": ("map exif",
                                 lambda c, f: api.decompress_resized(CTX, files(), OUT, threads=2, warp=M9.reshape(N, 3, 3) if c["map"] == 9 else M6,
                                                                     **mapped_keywords(c, "exif"))),
}


def all_cases():
    """(id, function name, case) of every function under every combination of its columns' values."""
    out = []
    for name, (columns, _) in FUNCTIONS.items():
        columns = columns.split()
        for values in itertools.product(*[range(len(COLUMNS_OF[c])) for c in columns]):
            case = {c: COLUMNS_OF[c][v] for c, v in zip(columns, values)}
            out.append(("%s[%s]" % (name, ",".join("%s=%d" % cv for cv in zip(columns, values))), name, case))
    return out


CASES = all_cases()

# Calls that are wrong twice: which complaint comes first.
WRONG = {
    "resize: filter, place": lambda: api.resize(CTX, pictures(), OUT, filter="lanczos", place="stretch"),
    "resize: orientations, place": lambda: api.resize(CTX, pictures(), OUT, orientations=[1], place="stretch"),
    "resize: anchor, fill": lambda: api.resize(CTX, pictures(), OUT, place="fit", anchor="left", fill=(1, 2)),
    "resize: place, images": lambda: api.resize(CTX, [torch.zeros(3, 3)], OUT, place=[(0, 0, 1, 1)] * 2),
    "resize_tensor: place, colour": lambda: api.resize_tensor(CTX, pictures(), OUT, SPEC(), place=[(0, 0, 1, 1)], colour=np.zeros((1, 12))),
    "resize_tensor: colour_clamp, flips": lambda: api.resize_tensor(CTX, pictures(), OUT, SPEC(), colour_clamp=(0, 1), flips=[1]),
    "resize_tensor: colour, images": lambda: api.resize_tensor(CTX, [torch.zeros(3, 3)], OUT, SPEC(), colour=np.zeros((2, 12))),
    "resize_tensor: images, flips": lambda: api.resize_tensor(CTX, [torch.zeros(3, 3)] * 2, OUT, SPEC(), flips=[1]),
    "warp: matrices, fill": lambda: api.warp(CTX, pictures(), M6[:1], OUT, fill=(1, 2)),
    "warp: edge, fill": lambda: api.warp(CTX, pictures(), M6, OUT, edge="wrap", fill=(1, 2)),
    "warp_tensor: fill, colour": lambda: api.warp_tensor(CTX, pictures(), M6, OUT, SPEC(), fill=(1, 2, 300), colour=np.zeros((1, 12))),
    "project_tensor: matrices, colour": lambda: api.project_tensor(CTX, pictures(), M9[:1], OUT, SPEC(), colour=np.zeros((1, 12))),
    "project_tensor: colour, flips": lambda: api.project_tensor(CTX, pictures(), M9, OUT, SPEC(), colour=np.zeros((1, 12)), flips=[1]),
    "decode_tensors: filter, planes": lambda: api.decode_tensors(CTX, (24, 16), batch()[1], batch()[2][:2], batch()[3], VIEWS, OUT, SPEC(),
                                                                 filter="nearest"),
    "decode_tensors: quanta, flips": lambda: api.decode_tensors(CTX, (24, 16), batch()[1], batch()[2], batch()[3][:1], VIEWS, OUT, SPEC(),
                                                                flips=[1]),
    "decode_resized_mixed: filter, views": lambda: api.decode_resized_mixed(CTX, spectrals(), VIEWS[:1], OUT, filter="nearest"),
    "decode_resized_mixed: views, orientations": lambda: api.decode_resized_mixed(CTX, spectrals(), VIEWS[:1], OUT, orientations=[1]),
    "decode_tensors_mixed: orientations, place": lambda: api.decode_tensors_mixed(CTX, spectrals(), VIEWS, OUT, SPEC(), orientations=[1, 300],
                                                                                    place="fill"),
    "decode_tensors_mixed: fill, colour": lambda: api.decode_tensors_mixed(CTX, spectrals(), VIEWS, OUT, SPEC(), place="fit", fill=(1, 2, -1),
                                                                             colour=np.zeros(12)),
    "decode_tensors_mixed: colour, flips": lambda: api.decode_tensors_mixed(CTX, spectrals(), VIEWS, OUT, SPEC(), colour=np.zeros(12),
                                                                              flips=[1]),
    "decode_crops_tensor_mixed: regions, orientations": lambda: api.decode_crops_tensor_mixed(CTX, spectrals(), CROPS[:1], OUT, SPEC(),
                                                                                                orientations=[1]),
    "decode_crops_tensor_mixed: orientations, place": lambda: api.decode_crops_tensor_mixed(CTX, spectrals(), CROPS, OUT, SPEC(),
                                                                                              orientations=[1], place=[(0, 0, 1, 1)]),
    "decode_warped_mixed: matrices, orientations": lambda: api.decode_warped_mixed(CTX, spectrals(), M6[:1], OUT, orientations=[1]),
    "decode_warped_mixed: orientations, edge": lambda: api.decode_warped_mixed(CTX, spectrals(), M6, OUT, orientations=[1], edge="wrap"),
    "decode_tensors_projected_mixed: fill, colour": lambda: api.decode_tensors_projected_mixed(CTX, spectrals(), M9, OUT, SPEC(), fill=(1, 2),
                                                                                                 colour_clamp=(0, 1)),
    "decompress_tensors: filter, regions": lambda: api.decompress_tensors(CTX, files(), OUT, SPEC(), filter="nearest",
                                                                           source_regions=CROPS[:1]),
    "decompress_tensors: regions, orientation": lambda: api.decompress_tensors(CTX, files(), OUT, SPEC(), source_regions=CROPS[:1],
                                                                                 orientation=[9000, 1]),
    "decompress_tensors: orientation, colour": lambda: api.decompress_tensors(CTX, files(), OUT, SPEC(), orientation=["exif"],
                                                                                colour_clamp=(0, 1)),
    "decompress_tensors: colour, warp rule": lambda: api.decompress_tensors(CTX, files(), OUT, SPEC(), colour=np.zeros(12), warp=M6,
                                                                              place="fit"),
    "decompress_tensors: warp rule, matrices": lambda: api.decompress_tensors(CTX, files(), OUT, SPEC(), warp=M6[:1], filter="bicubic"),
    "decompress_tensors: matrices, fill": lambda: api.decompress_tensors(CTX, files(), OUT, SPEC(), warp=M9[:1], fill=(1, 2)),
    "decompress_tensors: fill, flips": lambda: api.decompress_tensors(CTX, files(), OUT, SPEC(), warp=M6, fill=(1, 2), flips=[1]),
    "decompress_tensors: colour, place": lambda: api.decompress_tensors(CTX, files(), OUT, SPEC(), colour=np.zeros(12), place="stretch"),
    "decompress_tensors: place, flips": lambda: api.decompress_tensors(CTX, files(), OUT, SPEC(), place="fit", anchor="x", flips=[1]),
    "decompress_resized: orientation, warp rule": lambda: api.decompress_resized(CTX, files(), OUT, orientation=[1], warp=M6,
                                                                                   source_regions=CROPS),
    "decompress_resized: warp rule, edge": lambda: api.decompress_resized(CTX, files(), OUT, warp=M6, place="fit", edge="wrap"),
    "decompress_resized: orientation, place": lambda: api.decompress_resized(CTX, files(), OUT, orientation="exif" * 2, place=[(0, 0, 1, 1)]),
}


# ---- one call under the recorder --------------------------------------------------------------------------------------------------

def shape_of(result):
    """What came back, as JSON holds it: the kind, dtype and shape of every item, and the values of the host arrays."""
    items = result if isinstance(result, tuple) else (result,)
    out = []
    for r in items:
        if isinstance(r, torch.Tensor):
            out.append(["tensor", str(r.dtype), list(r.shape)])
        elif isinstance(r, np.ndarray):
            out.append(["array", str(r.dtype), list(r.shape), r.tolist()])
        else:
            out.append(["infos", len(r), all(isinstance(i, _lib.FrameInfo) for i in r)])
    return [isinstance(result, tuple), out]


def run(recorder, index, name, case):
    """-> (what the call returned, its one noted call: symbol, described arguments, raw pointers)."""
    recorder.calls.clear()
    result = FUNCTIONS[name][1](case, FILTERS[index % 3])
    assert len(recorder.calls) == 1, [c[0] for c in recorder.calls]
    return result, recorder.calls[0]


@pytest.fixture
def recorder(monkeypatch):
    files()                                                  # (made by the library itself, in front of the recorder)
    r = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: r)
    return r


@functools.lru_cache(maxsize=None)
def golden():
    """The record, unpacked: the file holds every distinct argument value once (`values`) and of a call its symbol, the index
    of each argument's value in the order of ARGS and that of what it returned."""
    with open(GOLDEN) as f:
        g = json.load(f)
    v = g["values"]
    calls = {ident: {"symbol": s, "args": {name: v[i] for name, i in zip(ARGS[s], args)}, "result": v[result]}
             for ident, (s, args, result) in g["calls"].items()}
    return {"calls": calls, "wrong": g["wrong"]}


def write_golden(calls, wrong):
    values, index = [], {}

    def ref(value):
        key = json.dumps(value, sort_keys=True)
        if key not in index:
            index[key] = len(values)
            values.append(key)
        return index[key]

    packed = ['%s: %s' % (json.dumps(ident), json.dumps([c["symbol"], [ref(c["args"][a]) for a in ARGS[c["symbol"]]], ref(c["result"])]))
              for ident, c in sorted(calls.items())]
    refusals = ['%s: %s' % (json.dumps(k), json.dumps(m)) for k, m in sorted(wrong.items())]
    with open(GOLDEN, "w") as f:                             # (one value, one call, one refusal per line)
        f.write('{"values": [\n%s\n],\n"calls": {\n%s\n},\n"wrong": {\n%s\n}}\n' % (",\n".join(values), ",\n".join(packed), ",\n".join(refusals)))


@pytest.mark.parametrize("index,ident,name,case", [(i,) + c for i, c in enumerate(CASES)], ids=[c[0] for c in CASES])
def test_one_wide_call_with_the_recorded_arguments(recorder, index, ident, name, case):
    want = golden()["calls"][ident]
    result, (symbol, args, raw) = run(recorder, index, name, case)
    wide, wide_args = widen(want["symbol"], want["args"])
    assert symbol == wide and symbol in CELLS
    assert list(args) == ARGS[symbol]
    for key in ARGS[symbol]:                                 # (one by one: the name of the first that differs shows)
        assert args[key] == wide_args[key], key
    assert shape_of(result) == want["result"]
    # the pointers: the output is the tensor that comes back, at its stride; the matrices applied are the array that comes back
    items = result if isinstance(result, tuple) else (result,)
    assert raw["out"] == items[0].data_ptr() and args["stride"] * N == items[0].numel() and items[0].is_contiguous()
    if "matrices_out" in raw:
        assert raw["matrices_out"] == items[-1].ctypes.data and items[-1].flags["C_CONTIGUOUS"]


def test_the_record_covers_every_cell_and_every_narrow_form():
    called = {c["symbol"] for c in golden()["calls"].values()}
    assert set(golden()["calls"]) == {c[0] for c in CASES}
    assert {WIDE.get(s, s) for s in called} == CELLS
    assert set(WIDE) <= called                               # every narrow form was what some case used to reach
    for narrow, wide in WIDE.items():
        assert set(ARGS[narrow]) <= set(ARGS[wide]), narrow


def test_the_tables_name_the_librarys_symbols():
    for symbol, names in ARGS.items():
        assert len(_lib.SIGNATURES[symbol][1]) == len(names), symbol


@pytest.mark.parametrize("ident", list(WRONG))
def test_a_call_wrong_twice_makes_the_recorded_complaint(recorder, ident):
    with pytest.raises(ValueError) as e:
        WRONG[ident]()
    assert str(e.value) == golden()["wrong"][ident]
    assert recorder.calls == []


# ---- run as a program: record the calls of the package as it stands, or time its argument building ------------------------------

def _record():
    files()
    r = Recorder(_lib.lib())
    _lib.lib = lambda: r
    calls, wrong = {}, {}
    for index, (ident, name, case) in enumerate(CASES):
        result, (symbol, args, raw) = run(r, index, name, case)
        calls[ident] = {"symbol": symbol, "args": args, "result": shape_of(result)}
    for ident, call in WRONG.items():
        try:
            call()
            raise AssertionError(ident)
        except ValueError as e:
            wrong[ident] = str(e)
    write_golden(calls, wrong)
    print(len(calls), "calls and", len(wrong), "refusals ->", GOLDEN)


def _time(reps=1000):
    """The host side alone: every case of the table, then decompress_tensors' argument building on 64 small files."""
    many = [synthetic_file("420", (16, 16), s)[0] for s in range(64)]
    r = Recorder(_lib.lib())
    _lib.lib = lambda: r
    t0 = time.perf_counter()
    for index, (ident, name, case) in enumerate(CASES):
        run(r, index, name, case)
    t1 = time.perf_counter()
    best = []
    for _ in range(5):
        t2 = time.perf_counter()
        for _ in range(reps // 5):
            r.calls.clear()
            api.decompress_tensors(CTX, many, OUT, SPEC(), orientation="exif", place="fit", flips=[0] * 64)
        best.append((time.perf_counter() - t2) / (reps // 5))
    print("every case of the table once: %.1f ms; decompress_tensors on 64 files, %d calls in 5 runs: %.1f .. %.1f us per call"
          % (1e3 * (t1 - t0), reps, 1e6 * min(best), 1e6 * max(best)))


if __name__ == "__main__":
    _time() if "--time" in sys.argv else _record()
