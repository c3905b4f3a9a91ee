"""Host-side mirror of the reference's hot-path interface over the C ABI.

Reference (tayloraswift/jpeg @ 2024_08_07, sources/jpeg/):
    JPEG.Data.Spectral.idct()                 decode.swift:4154
    JPEG.Data.Planar.interleaved(cosite:)     decode.swift:4182
    JPEG.Data.Rectangular.unpack(as:)         decode.swift:4294
    JPEG.Data.Rectangular.pack(size:layout:metadata:pixels:)   encode.swift:456
    JPEG.Data.Rectangular.decomposed()        encode.swift:389
    JPEG.Data.Planar.fdct(quanta:)            encode.swift:353
Same names, argument meaning and error behaviour (the reference's precondition failures
surface as JpegAmdError(EINVAL)).  PyTorch is used only to own device memory and the
stream; every computation is a call into libjpeg_amd.so.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

MAX_PLANES = _lib.MAX_PLANES


class YCbCr:
    """JPEG.YCbCr colour target (jpeg.swift:160-209, 481-540)."""
    code = _lib.COLOR_YCC8


class RGB:
    """JPEG.RGB colour target (jpeg.swift:210-269, 542-600)."""
    code = _lib.COLOR_RGB8


def _torch():
    import torch
    return torch


class Context:
    """One jpeg_amd_ctx bound to a device and to torch's current stream on it."""

    def __init__(self, device: int = 0, stream: Optional[int] = None, own_stream: bool = False, device_entropy: bool = False):
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError("jpeg_amd needs a GPU: torch.cuda.is_available() is False "
                               "(there is no CPU fallback)")
        self.device = int(device)
        self.torch_device = torch.device("cuda", self.device)
        if stream is None:
            stream = torch.cuda.current_stream(self.torch_device).cuda_stream
        self._h = C.c_void_p()
        flags = (_lib.CTX_OWN_STREAM if own_stream else 0) | (_lib.CTX_DEVICE_ENTROPY if device_entropy else 0)
        _lib.check(_lib.lib().jpeg_amd_ctx_create(self.device, C.c_void_p(stream), flags,
                                                 C.byref(self._h)), "jpeg_amd_ctx_create")

    @property
    def handle(self):
        return self._h

    @property
    def device_entropy_files(self) -> int:
        """Files this context has entropy-decoded on the GPU so far (jpeg_amd_ctx_device_entropy_files)."""
        n = C.c_int64()
        _lib.check(_lib.lib().jpeg_amd_ctx_device_entropy_files(self._h, C.byref(n)), "jpeg_amd_ctx_device_entropy_files")
        return n.value

    def synchronize(self):
        _lib.check(_lib.lib().jpeg_amd_ctx_synchronize(self._h), "synchronize", self._h)

    def timer_begin(self):
        _lib.check(_lib.lib().jpeg_amd_timer_begin(self._h), "timer_begin", self._h)

    def timer_end(self) -> float:
        ms = C.c_float()
        _lib.check(_lib.lib().jpeg_amd_timer_end(self._h, C.byref(ms)), "timer_end", self._h)
        return ms.value

    def empty(self, n: int, dtype):
        torch = _torch()
        return torch.empty(max(int(n), 0), dtype=dtype, device=self.torch_device)

    def upload(self, a: np.ndarray):
        """numpy (int16 / uint16 / uint8) -> device tensor (uint16 travels as int16)."""
        torch = _torch()
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint16:
            a = a.view(np.int16)
        return torch.from_numpy(a).to(self.torch_device)

    def close(self):
        if self._h:
            _lib.lib().jpeg_amd_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_DEFAULT: Dict[int, Context] = {}


def default_context(device: int = 0) -> Context:
    if device not in _DEFAULT:
        _DEFAULT[device] = Context(device)
    return _DEFAULT[device]


@dataclass(frozen=True)
class Component:
    """JPEG.Component + its quanta key (jpeg.swift:1107-1160)."""
    factor: Tuple[int, int]
    qi: int


class Layout:
    """The part of JPEG.Layout<Format> the spectral pipeline reads (jpeg.swift:1084-1635).

    format: 'y8' | 'ycc8' | ('custom', precision, n_recognized)
    components: {component key: Component(factor, qi)} in plane order.  Components beyond
    the format's recognised count are non-recognised: they take part in `scale` only.
    """

    def __init__(self, format, components: Dict[int, Component | tuple]):
        self.format = format
        comps = {}
        for key, c in components.items():
            if not isinstance(c, Component):
                factor, qi = c
                c = Component(tuple(factor), int(qi))
            comps[key] = c
        self.components = comps
        if format == "y8":
            self.precision, nrec = 8, 1
        elif format == "ycc8":
            self.precision, nrec = 8, 3
        elif isinstance(format, tuple) and format[0] == "custom":
            self.precision, nrec = int(format[1]), int(format[2])
        else:
            raise ValueError(f"unknown format {format!r}")
        if nrec > len(comps) or nrec > MAX_PLANES:
            raise ValueError("format recognises more components than the layout holds")
        self.recognized = list(comps.keys())[:nrec]
        self.planes = [comps[k] for k in self.recognized]

    @property
    def scale(self) -> Tuple[int, int]:
        """decode.swift:2181-2190: max factor over ALL components."""
        return (max(c.factor[0] for c in self.components.values()),
                max(c.factor[1] for c in self.components.values()))

    @property
    def count(self) -> int:
        return len(self.planes)

    def units(self, size) -> List[Tuple[int, int]]:
        """decode.swift:2606-2616"""
        sx, sy = self.scale

        def u(n, s):
            return n // s + (1 if n % s else 0)
        return [(u(size[0] * c.factor[0], 8 * sx), u(size[1] * c.factor[1], 8 * sy))
                for c in self.planes]

    def c_layout(self, size, units=None, q: Optional[Sequence[int]] = None) -> _lib.Layout:
        L = _lib.Layout()
        L.width, L.height = int(size[0]), int(size[1])
        L.precision, L.nplanes = self.precision, self.count
        L.scale_x, L.scale_y = self.scale
        units = units if units is not None else self.units(size)
        for p, c in enumerate(self.planes):
            L.factor_x[p], L.factor_y[p] = c.factor
            L.units_x[p], L.units_y[p] = units[p]
            L.qi[p] = q[p] if q is not None else 0
        return L


def _ptrs(tensors):
    return _lib.ptr_array([t.data_ptr() if t is not None else None for t in tensors])


def _quanta_array(tables: Sequence[np.ndarray]):
    q = np.ascontiguousarray(np.stack([np.asarray(t, np.uint16).reshape(64) for t in tables]))
    return q, q.ctypes.data_as(C.c_void_p)


class Spectral:
    """JPEG.Data.Spectral<Format> (decode.swift:1370-1479): quantised coefficients,
    one int16 tensor [units_y, units_x, 64] (zigzag) per plane, resident in HBM."""

    def __init__(self, ctx: Context, size, layout: Layout, planes, quanta: Sequence[np.ndarray],
                 q: Sequence[int]):
        self.ctx, self.size, self.layout = ctx, (int(size[0]), int(size[1])), layout
        self.planes = list(planes)
        self.quanta = [np.asarray(t, np.uint16).reshape(64).copy() for t in quanta]
        self.q = list(q)                     # Plane.q: table index per plane
        if len(self.planes) != layout.count or len(self.q) != layout.count:
            raise ValueError("plane count does not match layout")

    @classmethod
    def from_host(cls, ctx, size, layout, planes: Sequence[np.ndarray], quanta, q=None):
        q = list(q) if q is not None else _dedupe_q(layout)
        dev = [ctx.upload(np.asarray(p, np.int16)) for p in planes]
        return cls(ctx, size, layout, dev, quanta, q)

    @property
    def units(self):
        return [(int(p.shape[1]), int(p.shape[0])) for p in self.planes]

    def _layout(self):
        return self.layout.c_layout(self.size, self.units, self.q)

    def idct(self) -> "Planar":
        """Spectral.idct() -- decode.swift:4154-4165."""
        torch = _torch()
        L = self._layout()
        out = [self.ctx.empty(64 * ux * uy, torch.int16).view(8 * uy, 8 * ux)
               for ux, uy in self.units]
        qarr, qptr = _quanta_array(self.quanta)
        _lib.check(_lib.lib().jpeg_amd_spectral_idct(
            self.ctx.handle, C.byref(L), _ptrs(self.planes), qptr, len(self.quanta),
            _ptrs(out)), "jpeg_amd_spectral_idct", self.ctx.handle)
        return Planar(self.ctx, self.size, self.layout, out)

    def rectangular(self, cosite: bool = False) -> "Rectangular":
        """Fused idct().interleaved(cosite:) (decode.swift:4154-4165, 4182-4276) -> Rectangular: any format (precision 1 .. 16,
        1 .. 4 planes); one launch with no Planar in HBM where the planes lie at the image's scale or at half of it, the staged
        kernels otherwise -- the same samples either way."""
        torch = _torch()
        L = self._layout()
        W, H = self.size
        out = self.ctx.empty(W * H * self.layout.count, torch.int16)
        qarr, qptr = _quanta_array(self.quanta)
        _lib.check(_lib.lib().jpeg_amd_spectral_rectangular(
            self.ctx.handle, C.byref(L), _ptrs(self.planes), qptr, len(self.quanta), 1 if cosite else 0, out.data_ptr()),
            "jpeg_amd_spectral_rectangular", self.ctx.handle)
        return Rectangular(self.ctx, self.size, self.layout, out.view(H, W, self.layout.count))

    def decode(self, color=RGB, cosite: bool = False, region=None, scale: int = 1):
        """Fused idct().interleaved(cosite:).unpack(as:) -> uint8 tensor [H*W, 3].  region (x, y, width, height) in pixels,
        any alignment: the same decode cropped to it, bit for bit, as [height*width, 3] (jpeg_amd_decode_region).
        scale: the scale denominator 1 | 2 | 4 | 8: the image at 1/scale size straight from the coefficients, as
        [H'*W', 3] with (W', H') = scaled_size(size, scale) (jpeg_amd_decode_scaled).  Not together with region: a region of
        the scaled image is Spectral.view."""
        torch = _torch()
        L = self._layout()
        qarr, qptr = _quanta_array(self.quanta)
        if scale != 1:
            if region is not None:
                raise ValueError("region together with scale != 1: use Spectral.view")
            w, h = scaled_size(self.size, scale)
            out = self.ctx.empty(w * h * 3, torch.uint8)
            _lib.check(_lib.lib().jpeg_amd_decode_scaled(
                self.ctx.handle, C.byref(L), _ptrs(self.planes), qptr, len(self.quanta),
                1 if cosite else 0, color.code, int(scale), out.data_ptr()), "jpeg_amd_decode_scaled", self.ctx.handle)
            return out.view(-1, 3)
        if region is not None:
            reg = _region(region)
            r = reg._obj
            out = self.ctx.empty(max(r.width, 0) * max(r.height, 0) * 3, torch.uint8)
            _lib.check(_lib.lib().jpeg_amd_decode_region(
                self.ctx.handle, C.byref(L), _ptrs(self.planes), qptr, len(self.quanta),
                1 if cosite else 0, color.code, reg, out.data_ptr()), "jpeg_amd_decode_region", self.ctx.handle)
            return out.view(-1, 3)
        out = self.ctx.empty(self.size[0] * self.size[1] * 3, torch.uint8)
        _lib.check(_lib.lib().jpeg_amd_decode(
            self.ctx.handle, C.byref(L), _ptrs(self.planes), qptr, len(self.quanta),
            1 if cosite else 0, color.code, out.data_ptr()), "jpeg_amd_decode", self.ctx.handle)
        return out.view(-1, 3)

    def view(self, region, scale: int, color=RGB, cosite: bool = False, size=None, filter: str = "bilinear"):
        """The image at 1/scale size (scale 1 | 2 | 4 | 8, as decode(scale=)) cropped to region (x, y, width, height) in
        pixels of THAT image, any alignment, bit for bit, as uint8 [height, width, 3] (jpeg_amd_decode_view).  view_of_source
        turns a rectangle of the full-size image into such a region, view_denom picks the scale for a target size.
        size (Wt, Ht): that view bilinearly resampled to Wt x Ht, as uint8 [Ht, Wt, 3] (jpeg_amd_decode_resized);
        filter="antialias": resampled with the antialiasing filter instead (jpeg_amd_decode_resized_filter_batch on one
        image, the tables uploaded first); filter="bicubic": with the bicubic filter of decode_resized."""
        torch = _torch()
        L = self._layout()
        qarr, qptr = _quanta_array(self.quanta)
        v = _view(scale, region)
        code = _filter(filter)
        if size is not None:
            wt, ht = int(size[0]), int(size[1])
            out = self.ctx.empty(max(wt, 0) * max(ht, 0) * 3, torch.uint8)
            if code != _lib.FILTER_BILINEAR:
                dq = self.ctx.upload(np.stack(self.quanta).astype(np.uint16))
                _lib.check(_lib.lib().jpeg_amd_decode_resized_filter_batch(
                    self.ctx.handle, C.byref(L), 1, _ptrs(self.planes), _lib.size_array([0] * _lib.MAX_PLANES), dq.data_ptr(), 0,
                    len(self.quanta), 1 if cosite else 0, color.code, C.byref(v), wt, ht, code, out.data_ptr(), 0),
                    "jpeg_amd_decode_resized_filter_batch", self.ctx.handle)
                return out.view(ht, wt, 3)
            _lib.check(_lib.lib().jpeg_amd_decode_resized(
                self.ctx.handle, C.byref(L), _ptrs(self.planes), qptr, len(self.quanta),
                1 if cosite else 0, color.code, C.byref(v), wt, ht, out.data_ptr()), "jpeg_amd_decode_resized", self.ctx.handle)
            return out.view(ht, wt, 3)
        w, h = max(v.region.width, 0), max(v.region.height, 0)
        out = self.ctx.empty(w * h * 3, torch.uint8)
        _lib.check(_lib.lib().jpeg_amd_decode_view(
            self.ctx.handle, C.byref(L), _ptrs(self.planes), qptr, len(self.quanta),
            1 if cosite else 0, color.code, C.byref(v), out.data_ptr()), "jpeg_amd_decode_view", self.ctx.handle)
        return out.view(h, w, 3)

    def host_planes(self) -> List[np.ndarray]:
        return [p.cpu().numpy() for p in self.planes]

    def compress(self, scans, process: str = "baseline", metadata=None, path=None, restart_interval: int = 0) -> bytes:
        """Spectral.compress(stream:) / compress(path:) -- encode.swift:1918-1972, os.swift:330.
        scans: the layout's scan progression -- Scan objects, or plain lists of (plane index, dc
        selector, ac selector) for sequential scans; metadata: see _metadata_array.  The coefficient planes come back to the host and are entropy-coded
        there (csrc/entropy_encode.cpp).  Returns the file's bytes (and writes `path`)."""
        info = _lib.FrameInfo()
        info.width, info.height = self.size
        info.precision, info.ncomponents = self.layout.precision, self.layout.count
        info.process = {"baseline": 0, "extended": 1, "progressive": 2}[process]
        info.scale_x, info.scale_y = self.layout.scale
        info.restart_interval = int(restart_interval)   # extension: DRI + RSTm (0 = like the reference)
        keys = []
        for p, (key, comp) in enumerate(zip(self.layout.recognized, self.layout.planes)):
            info.id[p] = int(key)
            info.factor_x[p], info.factor_y[p] = comp.factor
            info.units_x[p], info.units_y[p] = self.units[p]
            keys.append(comp.qi)
        host = [np.ascontiguousarray(p.cpu().numpy()) for p in self.planes]
        # self.quanta[self.q[p]] is plane p's table; give every distinct quanta key one table
        tkeys = sorted(set(keys))
        tables = np.stack([self.quanta[self.q[keys.index(k)]] for k in tkeys]).astype(np.uint16)
        qkey = (C.c_int32 * len(keys))(*keys)
        tk = (C.c_int32 * len(tkeys))(*tkeys)
        sarr = _scan_array(scans)
        marr, nmeta, _keep = _metadata_array(metadata)
        n = C.c_size_t()
        args = [C.byref(info), qkey, _lib.ptr_array([h.ctypes.data for h in host]), tables.ctypes.data, tk, len(tkeys),
                sarr, len(scans), marr, nmeta]
        _lib.check(_lib.lib().jpeg_amd_jpeg_encode_spectral(*args, None, 0, C.byref(n)), "jpeg_amd_jpeg_encode_spectral")
        out = np.empty(n.value, np.uint8)
        _lib.check(_lib.lib().jpeg_amd_jpeg_encode_spectral(*args, out.ctypes.data, out.size, C.byref(n)),
                   "jpeg_amd_jpeg_encode_spectral")
        data = out.tobytes()
        if path is not None:
            with open(path, "wb") as f:
                f.write(data)
        return data

    def transform(self, op, region=None, requantize=None) -> "Spectral":
        """Lossless rotate / flip / crop / requantise, device to device (jpeg_amd_spectral_transform_batch; the contract is in
        include/jpeg_amd.h): what examples/rotate/main.swift and examples/recompress/main.swift do to a Spectral.
        op: a JPEG_AMD_XFORM_* value or name ("rot_ccw", "flip_h", ...; the reference's "ii", "iii", "iv").
        region: (x, y, width, height) in source pixels, applied before the op.  requantize: the new tables in OUTPUT
        orientation, {quanta key: 64 values} or one per entry of self.quanta; None keeps the coefficients exactly."""
        torch = _torch()
        op = _xform_op(op)
        L = self._layout()
        out = _lib.Layout()
        reg = _region(region)
        lib = _lib.lib()
        _lib.check(lib.jpeg_amd_transform_layout(C.byref(L), op, reg, C.byref(out)), "jpeg_amd_transform_layout")
        T = op & _lib.XFORM_TRANSPOSE
        comps = {k: Component((c.factor[1], c.factor[0]) if T else c.factor, c.qi) for k, c in self.layout.components.items()}
        layout = Layout(self.layout.format, comps)
        planes = [self.ctx.empty(64 * out.units_x[p] * out.units_y[p], torch.int16).view(out.units_y[p], out.units_x[p], 64)
                  for p in range(self.layout.count)]
        n = len(self.quanta)
        if requantize is None:
            quanta = [transform_quanta(op, t) for t in self.quanta]
        elif isinstance(requantize, dict):
            quanta = [transform_quanta(op, t) for t in self.quanta]
            for p, comp in enumerate(self.layout.planes):
                quanta[self.q[p]] = np.asarray(requantize[comp.qi], np.uint16).reshape(64)
        else:
            quanta = [np.asarray(t, np.uint16).reshape(64) for t in requantize]
            if len(quanta) != n:
                raise ValueError("requantize: one table per entry of self.quanta")
        d_q = self.ctx.upload(np.stack(self.quanta).astype(np.uint16))
        d_qo = self.ctx.upload(np.stack(quanta).astype(np.uint16)) if requantize is not None else None
        flag = torch.zeros(1, dtype=torch.int32, device=self.ctx.torch_device)
        zero = _lib.size_array([0] * MAX_PLANES)
        _lib.check(lib.jpeg_amd_spectral_transform_batch(
            self.ctx.handle, C.byref(L), 1, op, reg, _ptrs(self.planes), zero, d_q.data_ptr(), 0, n,
            d_qo.data_ptr() if d_qo is not None else None, _ptrs(planes), zero, flag.data_ptr()),
            "jpeg_amd_spectral_transform_batch", self.ctx.handle)
        if int(flag.item()):
            raise _lib.JpegAmdError(_lib.EINVAL, "Spectral.transform: a coefficient the reference would trap on "
                                                 "(Int16 overflow, q_in > 32767 or q_out = 0)")
        return Spectral(self.ctx, (out.width, out.height), layout, planes, quanta, self.q)

    def reduce(self, denom: int, quanta=None) -> "Spectral":
        """This image at 1/denom size (denom 2 | 4 | 8), coefficients to coefficients, device to device, in one launch
        (jpeg_amd_spectral_reduce_batch; the contract is in include/jpeg_amd.h, "spectral reduce"): every plane's scaled-decode
        samples through Spectral.Plane.fdct -- no interleave and no colour conversion, any layout and precision.
        quanta: the output tables, {quanta key: 64 values} or one per entry of self.quanta; None keeps the input's."""
        torch = _torch()
        L = self._layout()
        out = _lib.Layout()
        lib = _lib.lib()
        _lib.check(lib.jpeg_amd_reduce_layout(C.byref(L), int(denom), C.byref(out)), "jpeg_amd_reduce_layout")
        n = len(self.quanta)
        tables = [np.asarray(t, np.uint16).reshape(64) for t in self.quanta]
        if isinstance(quanta, dict):
            for p, comp in enumerate(self.layout.planes):
                tables[self.q[p]] = np.asarray(quanta[comp.qi], np.uint16).reshape(64)
        elif quanta is not None:
            tables = [np.asarray(t, np.uint16).reshape(64) for t in quanta]
            if len(tables) != n:
                raise ValueError("quanta: one table per entry of self.quanta")
        if any((tables[t] == 0).any() for t in set(self.q)):
            raise _lib.JpegAmdError(_lib.EINVAL, "Spectral.reduce: a zero in an output table")
        planes = [self.ctx.empty(64 * out.units_x[p] * out.units_y[p], torch.int16).view(out.units_y[p], out.units_x[p], 64)
                  for p in range(self.layout.count)]
        d_q = self.ctx.upload(np.stack(self.quanta).astype(np.uint16))
        d_qo = self.ctx.upload(np.stack(tables).astype(np.uint16)) if quanta is not None else None
        zero = _lib.size_array([0] * MAX_PLANES)
        _lib.check(lib.jpeg_amd_spectral_reduce_batch(
            self.ctx.handle, C.byref(L), 1, int(denom), _ptrs(self.planes), zero, d_q.data_ptr(), 0, n,
            d_qo.data_ptr() if d_qo is not None else None, _ptrs(planes), zero),
            "jpeg_amd_spectral_reduce_batch", self.ctx.handle)
        return Spectral(self.ctx, (out.width, out.height), self.layout, planes, tables, self.q)

    def set(self, width: Optional[int] = None, height: Optional[int] = None) -> None:
        """Spectral.set(width:) / set(height:) (decode.swift:2443-2500), in place: the image is cropped or grows from its
        top left corner; new blocks are zero."""
        w = self.size[0] if width is None else int(width)
        h = self.size[1] if height is None else int(height)
        t = self.transform(0, (0, 0, w, h))
        self.size, self.planes = t.size, t.planes

    @staticmethod
    def _file_layout(info) -> Layout:
        n = info.ncomponents
        if info.precision == 8 and n == 1:
            fmt = "y8"
        elif info.precision == 8 and n == 3:
            fmt = "ycc8"
        else:
            fmt = ("custom", info.precision, n)
        return Layout(fmt, {info.id[c]: Component((info.factor_x[c], info.factor_y[c]), c) for c in range(n)})

    @classmethod
    def decompress(cls, ctx: Context, source, scans: int = 0, entropy: str = "host") -> "Spectral":
        """Spectral.decompress(stream:) / decompress(path:) -- decode.swift:3728, os.swift:309.
        source: a path or the file's bytes.  entropy="host": the entropy-coded segments are decoded on the host by the
        library (csrc/entropy.cpp) and the coefficient planes uploaded; entropy="device": the file's bytes go up and its
        restart intervals are decoded on the GPU (jpeg_amd_jpeg_decode_spectral_device; sequential files whose restart
        markers are all in place -- plan_intervals says which)."""
        if entropy == "device":
            if scans:
                raise ValueError("entropy='device' decodes whole files")
            return decompress_spectrals(ctx, [source])[0]
        if entropy != "host":
            raise ValueError("entropy is 'host' or 'device'")
        data = _file_bytes(source)
        info, planes, quanta = _decode_spectral(data, scans)   # scans > 0: the image after that many scans
        n = info.ncomponents
        return cls.from_host(ctx, (info.width, info.height), cls._file_layout(info), planes, [quanta[c] for c in range(n)],
                             q=list(range(n)))


class Scan:
    """JPEG.Header.Scan constructors (jpeg.swift:1640-1760).  Components are PLANE INDICES
    (frame order); table selectors are 0..3."""

    def __init__(self, components, band=(0, 0), bit=0, refine=0):
        self.components, self.band, self.bit, self.refine = sorted(components), band, bit, refine

    @classmethod
    def sequential(cls, *components):
        """.sequential((c, dc, ac), ...)"""
        return cls(components)

    @classmethod
    def progressive_dc(cls, *components, bits):
        """.progressive((c, dc), ..., bits: bits...)"""
        return cls([(c, dc, 0) for c, dc in components], (0, 1), bits, 0)

    @classmethod
    def progressive_dc_refine(cls, *components, bit):
        """.progressive(c, ..., bit: bit)"""
        return cls([(c, 0, 0) for c in components], (0, 1), bit, 1)

    @classmethod
    def progressive_ac(cls, component, band, bits):
        """.progressive((c, ac), band: lo ..< hi, bits: bits...)"""
        return cls([(component[0], 0, component[1])], (max(band[0], 1), min(band[1], 64)), bits, 0)

    @classmethod
    def progressive_ac_refine(cls, component, band, bit):
        """.progressive((c, ac), band: lo ..< hi, bit: bit)"""
        return cls([(component[0], 0, component[1])], (max(band[0], 1), min(band[1], 64)), bit, 1)


def _scan_array(scans):
    """Scan objects, or plain [(plane index, dc selector, ac selector), ...] lists for
    sequential scans -> jpeg_amd_scan[]."""
    arr = (_lib.Scan * len(scans))()
    for i, sc in enumerate(scans):
        if not isinstance(sc, Scan):
            sc = Scan.sequential(*sc)
        arr[i].ncomponents = len(sc.components)
        for j, (c, dc, ac) in enumerate(sc.components):
            arr[i].component[j], arr[i].dc[j], arr[i].ac[j] = c, dc, ac
        arr[i].band_lo, arr[i].band_hi = sc.band
        arr[i].bit, arr[i].refine = sc.bit, sc.refine
    return arr


def _metadata_array(metadata):
    """[("jfif", (version_minor, unit, density_x, density_y)) | ("comment", bytes) |
    ("application", n, bytes), ...] -> (jpeg_amd_metadata[], keep-alive buffers) -- JPEG.Metadata."""
    metadata = list(metadata or [])
    arr = (_lib.Metadata * max(len(metadata), 1))()
    keep = []
    for i, m in enumerate(metadata):
        if m[0] == "jfif":
            arr[i].kind = 0
            arr[i].jfif.version_minor, arr[i].jfif.unit, arr[i].jfif.density_x, arr[i].jfif.density_y = m[1]
        else:
            data = np.frombuffer(bytes(m[-1]), np.uint8).copy()
            keep.append(data)
            arr[i].kind, arr[i].app = (2, 0) if m[0] == "comment" else (1, int(m[1]))
            arr[i].data, arr[i].size = data.ctypes.data, data.size
    return arr, len(metadata), keep


def _file_bytes(source) -> np.ndarray:
    if isinstance(source, np.ndarray):
        return np.ascontiguousarray(source, np.uint8)
    if isinstance(source, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(source), np.uint8)
    return np.fromfile(source, np.uint8)       # a path


def inspect(source) -> _lib.FrameInfo:
    """Frame geometry of a JPEG file without decoding its scans (jpeg_amd_jpeg_inspect)."""
    data = _file_bytes(source)
    info = _lib.FrameInfo()
    _lib.check(_lib.lib().jpeg_amd_jpeg_inspect(data.ctypes.data, data.size, C.byref(info)), "jpeg_amd_jpeg_inspect")
    return info


def plan_intervals(source):
    """Whether a file's entropy decoding can run on the GPU, and how much work it is (jpeg_amd_jpeg_plan_intervals):
    -> (info, nscans, nintervals), or raises with the planner's status (ENOSUP: the host decodes this file)."""
    data = _file_bytes(source)
    info, nscans, nintervals = _lib.FrameInfo(), C.c_int32(), C.c_int64()
    _lib.check(_lib.lib().jpeg_amd_jpeg_plan_intervals(data.ctypes.data, data.size, C.byref(info), C.byref(nscans), C.byref(nintervals)),
               "jpeg_amd_jpeg_plan_intervals")
    return info, nscans.value, nintervals.value


def decompress_spectrals(ctx: "Context", sources) -> List["Spectral"]:
    """Files of any mix of sizes and layouts -> Spectral images, entropy-decoded on the GPU in one launch
    (jpeg_amd_jpeg_decode_spectral_device).  Raises if the planner refuses any of the files, with nothing decoded."""
    torch = _torch()
    files = [_file_bytes(s) for s in sources]
    n = len(files)
    if n == 0:
        return []
    infos = [inspect(f) for f in files]
    planes = [[torch.empty((i.units_y[c], i.units_x[c], 64), dtype=torch.int16, device=ctx.torch_device) for c in range(i.ncomponents)]
              for i in infos]
    coef = (C.c_void_p * (MAX_PLANES * n))()
    for k, ps in enumerate(planes):
        for c, t in enumerate(ps):
            coef[MAX_PLANES * k + c] = t.data_ptr()
    quanta = np.zeros((n, MAX_PLANES, 64), np.uint16)
    out_info, status = (_lib.FrameInfo * n)(), (C.c_int32 * n)()
    _lib.check(_lib.lib().jpeg_amd_jpeg_decode_spectral_device(
        ctx.handle, n, (C.c_void_p * n)(*[f.ctypes.data for f in files]), (C.c_size_t * n)(*[f.size for f in files]), coef,
        quanta.ctypes.data, out_info, status), "jpeg_amd_jpeg_decode_spectral_device", ctx.handle)
    return [Spectral(ctx, (i.width, i.height), Spectral._file_layout(i), planes[k], [quanta[k][c] for c in range(i.ncomponents)],
                     q=list(range(i.ncomponents))) for k, i in enumerate(out_info)]


def exif_orientation(source) -> int:
    """The EXIF orientation of a JPEG file (a path or its bytes), 1 .. 8 (jpeg_amd_jpeg_orientation): IFD0's tag 0x0112 of the
    first Exif APP1 segment in front of the first scan; 1 where there is none, or none that is well-formed."""
    data = _file_bytes(source)
    o = C.c_int32()
    _lib.check(_lib.lib().jpeg_amd_jpeg_orientation(data.ctypes.data, data.size, C.byref(o)), "jpeg_amd_jpeg_orientation")
    return int(o.value)


def orient_region(orientation: int, size, region=None) -> Tuple[int, int, int, int]:
    """A rectangle (x, y, width, height) of the ORIENTED image of a stored image of size (w, h) -- None: the whole of it -- as
    the stored rectangle that holds its pixels (jpeg_amd_orient_region; include/jpeg_amd.h, "oriented resample")."""
    r = _lib.Region()
    _lib.check(_lib.lib().jpeg_amd_orient_region(int(orientation), int(size[0]), int(size[1]), _region(region), C.byref(r)),
               "jpeg_amd_orient_region")
    return r.x, r.y, r.width, r.height


def _orientations(orientations, n: int, exif: bool = False):
    """orientations=... of the resample calls -> the c bytes for h_orient, or None (every image as it is stored).  exif: the file
    calls, where "exif" (the whole call, or an entry of a sequence) is JPEG_AMD_ORIENT_EXIF."""
    if orientations is None:
        return None
    if isinstance(orientations, str):
        orientations = [orientations] * n
    vals = [_lib.ORIENT_EXIF if exif and isinstance(o, str) and o.lower() == "exif" else o for o in orientations]
    if len(vals) != n or any(isinstance(o, str) or not 0 <= int(o) <= 255 for o in vals):
        raise ValueError("orientations: one value in 1 .. 8 per image" + (', or "exif"' if exif else ""))
    return (C.c_uint8 * max(n, 1))(*[int(o) for o in vals])


_PLACE_MODES = {"fit": _lib.PLACE_FIT, "fit-down": _lib.PLACE_FIT_DOWN, "fit_down": _lib.PLACE_FIT_DOWN}
_ANCHORS = {"centre": _lib.ANCHOR_CENTRE, "center": _lib.ANCHOR_CENTRE, "top-left": _lib.ANCHOR_TOP_LEFT,
            "top_left": _lib.ANCHOR_TOP_LEFT}


def _anchor(anchor) -> int:
    if isinstance(anchor, str) and anchor.lower() in _ANCHORS:
        return _ANCHORS[anchor.lower()]
    raise ValueError('anchor: "centre" or "top-left"')


def place_window(mode, src_size, out_size, anchor="centre") -> Tuple[int, int, int, int]:
    """The window (x, y, width, height) that place="fit" / "fit-down" gives a source of src_size (w, h) on a canvas of out_size
    (Wt, Ht) (jpeg_amd_place_window; include/jpeg_amd.h, "placed resample"): aspect-preserving, "fit-down" never enlarging."""
    if not (isinstance(mode, str) and mode.lower() in _PLACE_MODES):
        raise ValueError('place_window: mode "fit" or "fit-down"')
    r = _lib.Region()
    _lib.check(_lib.lib().jpeg_amd_place_window(_PLACE_MODES[mode.lower()], _anchor(anchor), int(src_size[0]), int(src_size[1]),
                                                int(out_size[0]), int(out_size[1]), C.byref(r)), "jpeg_amd_place_window")
    return r.x, r.y, r.width, r.height


def _placement(place, anchor, fill, n: int):
    """place=, anchor=, fill= of the resample calls -> (struct jpeg_amd_placement, room for the applied windows, keep), or
    (None, None, None) for place=None.  place: "fit", "fit-down" or one (x, y, width, height) per image."""
    if place is None:
        return None, None, None
    p = _lib.Placement()
    p.anchor = _anchor(anchor)
    keep = None
    if isinstance(place, str):
        if place.lower() not in _PLACE_MODES:
            raise ValueError('place: None, "fit", "fit-down" or one (x, y, width, height) per image')
        p.mode = _PLACE_MODES[place.lower()]
    else:
        w = np.asarray(place, np.int64).reshape(-1, 4)
        if w.shape[0] != n:
            raise ValueError("place: one (x, y, width, height) per image")
        keep = (_lib.Region * max(n, 1))()
        for i, r in enumerate(w.tolist()):
            keep[i].x, keep[i].y, keep[i].width, keep[i].height = r
        p.mode = _lib.PLACE_WINDOWS
        p.h_windows = C.cast(keep, C.c_void_p)
    f = [int(v) for v in fill]
    if len(f) != 3 or min(f) < 0 or max(f) > 255:
        raise ValueError("fill: three bytes")
    p.fill[0], p.fill[1], p.fill[2] = f
    return p, (_lib.Region * max(n, 1))(), keep


_EDGES = {"fill": _lib.EDGE_FILL, "replicate": _lib.EDGE_REPLICATE}


def _warp(edge, fill) -> "_lib.Warp":
    """edge=, fill= of the warp calls -> struct jpeg_amd_warp."""
    w = _lib.Warp()
    if isinstance(edge, str):
        if edge.lower() not in _EDGES:
            raise ValueError('edge: "fill" or "replicate"')
        w.edge = _EDGES[edge.lower()]
    else:
        w.edge = int(edge)          # (the library judges it)
    f = [int(v) for v in fill]
    if len(f) != 3 or min(f) < 0 or max(f) > 255:
        raise ValueError("fill: three bytes")
    w.fill[0], w.fill[1], w.fill[2] = f
    return w


def _matrices(matrices, n: int, k: int = 6) -> np.ndarray:
    """matrices= of the warp calls (k = 6 numbers each) and of the project calls (k = 9) -> float32 [n, k], contiguous."""
    m = np.ascontiguousarray(np.asarray(matrices, np.float32).reshape(-1, k))
    if m.shape[0] != n:
        raise ValueError("matrices: one (m00, m01, m02, m10, m11, m12%s) per image" % (", m20, m21, m22" if k == 9 else ""))
    return m


def _pad_affine(m: np.ndarray) -> np.ndarray:
    """[n, 6] affine matrices as [n, 9] homographies with the last row (0, 0, 1): the same map ("bicubic warp")."""
    return np.ascontiguousarray(np.concatenate([m, np.tile(np.array([0.0, 0.0, 1.0], np.float32), (m.shape[0], 1))], axis=1))


def _map_view(k: int, size, layout: "Layout", matrix, out_size, orientation: int, filter: str = "bilinear"):
    """warp_view (k = 6) and project_view (k = 9); with the bicubic filter both through jpeg_amd_project_filter_view."""
    code = _map_filter(filter)
    m = _matrices(matrix, 1, k)
    v = _lib.View()
    L = layout.c_layout(size)
    if code == _lib.FILTER_BILINEAR:
        name = "jpeg_amd_project_view" if k == 9 else "jpeg_amd_warp_view"
        mv = np.zeros(k, np.float32)
        _lib.check(getattr(_lib.lib(), name)(C.byref(L), int(orientation), m.ctypes.data, int(out_size[0]), int(out_size[1]), C.byref(v),
                                             mv.ctypes.data), name)
    else:
        name = "jpeg_amd_project_filter_view"
        m = m if k == 9 else _pad_affine(m)
        mv = np.zeros(9, np.float32)
        _lib.check(getattr(_lib.lib(), name)(C.byref(L), int(orientation), m.ctypes.data, code, int(out_size[0]), int(out_size[1]),
                                             C.byref(v), mv.ctypes.data), name)
        mv = mv[:k].copy()
    return (v.denom, v.region.x, v.region.y, v.region.width, v.region.height), mv


def _cos_sin_degrees(angle: float) -> Tuple[float, float]:
    """(cos, sin) of an angle in degrees, exact at the multiples of 90."""
    a = math.fmod(float(angle), 360.0)
    if a % 90.0 == 0.0:
        return [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][int(a // 90.0) % 4]
    return math.cos(math.radians(a)), math.sin(math.radians(a))


def affine_matrix(src_size, out_size, angle: float = 0.0, scale: float = 1.0, shear=(0.0, 0.0), translate=(0.0, 0.0),
                  source_region=None) -> np.ndarray:
    """The matrix of the warp calls (include/jpeg_amd.h, "warped resample") for the usual augmentation parameters: the INVERSE
    map that takes the centre of the out_size (Wt, Ht) canvas to the centre of source_region (x, y, width, height) of an image
    of src_size (w, h) -- None: the whole image.  The canvas is rotated by `angle` degrees counter-clockwise about its centre,
    sheared by `shear` degrees (torchvision's convention and formulas: the inverse of RSS), scaled by `scale` and moved by
    `translate` canvas pixels, and then stretched onto the rectangle, so that angle = 0, shear = 0, scale = 1, translate = 0 is
    exactly the crop-resize (width / Wt, 0, x, 0, height / Ht, y).  Computed in double, returned as float32 [6]."""
    x0, y0, w, h = (0, 0, int(src_size[0]), int(src_size[1])) if source_region is None else (int(v) for v in source_region)
    wt, ht = int(out_size[0]), int(out_size[1])
    if w < 1 or h < 1 or wt < 1 or ht < 1 or not scale > 0.0:
        raise ValueError("affine_matrix: sizes of at least 1 and a positive scale")
    sx, sy = math.radians(float(shear[0])), math.radians(float(shear[1]))
    # torchvision's _get_inverse_affine_matrix; its angle is clockwise, so rot = -angle
    c, s = _cos_sin_degrees(-float(angle) - float(shear[1]))
    c0, s0 = _cos_sin_degrees(-float(angle))
    a = c / math.cos(sy)
    b = -c * math.tan(sx) / math.cos(sy) - s0
    cc = s / math.cos(sy)
    d = -s * math.tan(sx) / math.cos(sy) + c0
    l00, l01, l10, l11 = d / scale, -b / scale, -cc / scale, a / scale
    px, py = wt / 2.0 + float(translate[0]), ht / 2.0 + float(translate[1])
    p = l00 * px + l01 * py
    q = l10 * px + l11 * py
    m = [w * l00 / wt, w * l01 / wt, (x0 + w / 2.0) - w * p / wt, h * l10 / ht, h * l11 / ht, (y0 + h / 2.0) - h * q / ht]
    return np.array([v + 0.0 for v in m], np.float64).astype(np.float32)


def warp_view(size, layout: "Layout", matrix, out_size, orientation: int = 1, filter: str = "bilinear"):
    """The view that a warp of an image of `size` (w, h) and `layout` reads, and the matrix against it (jpeg_amd_warp_view):
    `matrix` (6 values) maps the centres of the out_size (Wt, Ht) canvas into the UPRIGHT image, the stored image seen through
    `orientation` 1 .. 8.  filter: "bilinear", or "bicubic" for the view of warp(filter="bicubic"), one pixel wider on each
    side (jpeg_amd_project_filter_view on the matrix with the last row (0, 0, 1)).
    Returns ((denom, x, y, width, height), float32 [6])."""
    return _map_view(6, size, layout, matrix, out_size, orientation, filter)


def perspective_matrix(src_points, out_points) -> np.ndarray:
    """The matrix of the project calls (include/jpeg_amd.h, "projective resample") that takes four points of the canvas,
    out_points [(x, y)] * 4 in continuous pixel coordinates, to four points of the source, src_points: the INVERSE map of
    torchvision's perspective(startpoints=src_points, endpoints=out_points), with m22 = 1.  The eight unknowns are solved in
    float64 and returned as float64 [3, 3] (the calls round to float32); ValueError for a singular system (three points on a
    line, or a map whose m22 would be 0).  Two axis-aligned rectangles, the corners in the same order, give exactly
    (sx, 0, x0, 0, sy, y0, 0, 0, 1)."""
    src = np.asarray(src_points, np.float64).reshape(-1, 2)
    out = np.asarray(out_points, np.float64).reshape(-1, 2)
    if src.shape != (4, 2) or out.shape != (4, 2) or not (np.isfinite(src).all() and np.isfinite(out).all()):
        raise ValueError("perspective_matrix: four finite (x, y) points each")

    def rectangle(p):   # corners in the order (x0, y0), (x1, y0), (x1, y1), (x0, y1) or (x0, y0), (x1, y0), (x0, y1), (x1, y1)
        (ax, ay), (bx, by), (cx, cy), (dx, dy) = p.tolist()
        if ay == by and ax != bx and bx == cx and cy == dy and dx == ax and cy != ay:
            return ax, ay, bx, cy, 0
        if ay == by and ax != bx and ax == cx and bx == dx and cy == dy and cy != ay:
            return ax, ay, bx, cy, 1
        return None

    rs, ro = rectangle(src), rectangle(out)
    if rs is not None and ro is not None and rs[4] == ro[4]:
        sx, sy = (rs[2] - rs[0]) / (ro[2] - ro[0]), (rs[3] - rs[1]) / (ro[3] - ro[1])
        return np.array([[sx, 0.0, rs[0] - sx * ro[0]], [0.0, sy, rs[1] - sy * ro[1]], [0.0, 0.0, 1.0]], np.float64)
    a = np.zeros((8, 8), np.float64)
    b = np.zeros(8, np.float64)
    for k in range(4):
        (x, y), (u, v) = out[k], src[k]
        a[2 * k] = [x, y, 1.0, 0.0, 0.0, 0.0, -u * x, -u * y]
        a[2 * k + 1] = [0.0, 0.0, 0.0, x, y, 1.0, -v * x, -v * y]
        b[2 * k], b[2 * k + 1] = u, v
    scale = np.abs(a).max(axis=0)
    if not (scale > 0.0).all() or np.linalg.cond(a / scale) > 1e12:
        raise ValueError("perspective_matrix: the points do not determine a projective map")
    h = np.linalg.solve(a / scale, b) / scale
    if not np.isfinite(h).all():
        raise ValueError("perspective_matrix: the points do not determine a projective map")
    return np.append(h, 1.0).reshape(3, 3)


def project_view(size, layout: "Layout", matrix, out_size, orientation: int = 1, filter: str = "bilinear"):
    """The view that a projective map of an image of `size` (w, h) and `layout` reads, and the matrix against it
    (jpeg_amd_project_view): `matrix` (9 values, or [3, 3]) maps the centres of the out_size (Wt, Ht) canvas into the UPRIGHT
    image, the stored image seen through `orientation` 1 .. 8.  filter: as in warp_view (jpeg_amd_project_filter_view).
    Returns ((denom, x, y, width, height), float32 [9])."""
    return _map_view(9, size, layout, matrix, out_size, orientation, filter)


_GREY = (0.2989, 0.587, 0.114)                     # torchvision's rgb_to_grayscale
_RGB_TO_YIQ = ((0.299, 0.587, 0.114), (0.5959, -0.2746, -0.3213), (0.2115, -0.5227, 0.3112))


def colour_matrix(brightness: float = 1.0, contrast: float = 1.0, saturation: float = 1.0, hue: float = 0.0, pivot: float = 128.0,
                  grey: bool = False, order: str = "rgb") -> np.ndarray:
    """One image's matrix for colour= of the tensor calls (include/jpeg_amd.h, "colour stage"): float32 [3, 4], row c the
    three factors of (R, G, B) and the offset of output channel c, in byte units.  The four jitter operations compose into
    B . C . S . H, the hue rotation applied to the pixel first:
      hue: a rotation of the I/Q plane of YIQ by `hue` TURNS (I' = cos I - sin Q, Q' = sin I + cos Q), written as
        identity + inverse(T) (R - identity) T so that hue = 0 is the identity exactly;
      saturation: s x + (1 - s) L x, every row of L torchvision's grey weights (0.2989, 0.587, 0.114): the linear form of
        adjust_saturation (which clamps to the value range afterwards; here colour_clamp does that, once, at the end);
      contrast: c x + (1 - c) pivot.  torchvision's adjust_contrast pivots on the grey mean of the image itself, which this
        stage cannot know: the caller supplies `pivot` (the default is mid-grey; pass the image's mean to match torchvision);
      brightness: b x.
    grey: every output channel is L of the result (RandomGrayscale); order "bgr": the output channels reversed.  Both are
    multiplied on from the left, last.  Composed in double and rounded to float32 once; the defaults give the identity exactly."""
    if order not in ("rgb", "bgr"):
        raise ValueError('order: "rgb" or "bgr"')

    def affine(lin, offset=(0.0, 0.0, 0.0)):
        m = np.eye(4)
        m[:3, :3] = lin
        m[:3, 3] = offset
        return m

    t = np.array(_RGB_TO_YIQ, np.float64)
    a = 2.0 * math.pi * float(hue)
    rot = np.array([[0.0, 0.0, 0.0], [0.0, math.cos(a) - 1.0, -math.sin(a)], [0.0, math.sin(a), math.cos(a) - 1.0]])
    luma = np.array([_GREY] * 3, np.float64)
    s, c, b = float(saturation), float(contrast), float(brightness)
    h_m = affine(np.eye(3) + np.linalg.inv(t) @ rot @ t)
    s_m = affine(s * np.eye(3) + (1.0 - s) * luma)
    c_m = affine(c * np.eye(3), [(1.0 - c) * float(pivot)] * 3)
    b_m = affine(b * np.eye(3))
    m = b_m @ c_m @ s_m @ h_m
    if grey:
        m = affine(luma) @ m
    if order == "bgr":
        m = affine(np.eye(3)[::-1]) @ m
    return np.ascontiguousarray((m[:3] + 0.0).astype(np.float32))


def _colour(colour, colour_clamp, n: int):
    """colour=, colour_clamp= of the tensor calls -> (struct jpeg_amd_colour, keep), or (None, None) for colour=None.
    colour: [n, 3, 4] or [n, 12]; colour_clamp: (lo, hi) in byte units, None: no clamp."""
    if colour is None:
        if colour_clamp is not None:
            raise ValueError("colour_clamp: only together with colour")
        return None, None
    k = np.ascontiguousarray(np.asarray(colour, np.float32).reshape(-1, 12))
    if k.shape[0] != n:
        raise ValueError("colour: one matrix [3, 4] per image")
    lo, hi = (-math.inf, math.inf) if colour_clamp is None else (float(colour_clamp[0]), float(colour_clamp[1]))
    c = _lib.Colour()
    c.h_matrices, c.lo, c.hi = k.ctypes.data, lo, hi
    return c, k


def _decode_spectral(data: np.ndarray, scans: int = 0):
    info = inspect(data)
    planes = [np.empty((info.units_y[c], info.units_x[c], 64), np.int16) for c in range(info.ncomponents)]
    quanta = np.zeros((MAX_PLANES, 64), np.uint16)
    _lib.check(_lib.lib().jpeg_amd_jpeg_decode_spectral_partial(
        data.ctypes.data, data.size, _lib.ptr_array([p.ctypes.data for p in planes]), quanta.ctypes.data, None, 0, scans),
        "jpeg_amd_jpeg_decode_spectral_partial")
    return info, planes, quanta


def _xform_op(op) -> int:
    """JPEG_AMD_XFORM_* value or name ("none", "transpose", "flip_h", "flip_v", "rot_180", "rot_ccw", "rot_cw",
    "transverse"; the reference's rotations "ii", "iii", "iv")."""
    if isinstance(op, str):
        key = op.lower()
        if key not in _lib.XFORM:
            raise ValueError(f"unknown transform {op!r}")
        return _lib.XFORM[key]
    op = int(op)
    if not 0 <= op <= 7:
        raise ValueError(f"transform op {op} is not in 0 .. 7")
    return op


def _region(region):
    if region is None:
        return None
    r = _lib.Region()
    r.x, r.y, r.width, r.height = (int(v) for v in region)
    return C.byref(r)


def _view(denom, region) -> "_lib.View":
    v = _lib.View()
    v.denom = int(denom)
    v.region.x, v.region.y, v.region.width, v.region.height = (int(t) for t in region)
    return v


def _views(views):
    """views [n, 5] of (denom, x, y, width, height) -> (them as int32 [n, 5], the c views)."""
    vs = np.ascontiguousarray(np.asarray(views, np.int32).reshape(-1, 5))
    h_views = (_lib.View * max(vs.shape[0], 1))()
    for i, row in enumerate(vs.tolist()):
        h_views[i] = _view(row[0], row[1:])
    return vs, h_views


def transform_quanta(op, table) -> np.ndarray:
    """q_out[z] = q_in[m(z)] (jpeg_amd_transform_quanta)."""
    t = np.ascontiguousarray(np.asarray(table, np.uint16).reshape(64))
    out = np.empty(64, np.uint16)
    _lib.check(_lib.lib().jpeg_amd_transform_quanta(_xform_op(op), t.ctypes.data, out.ctypes.data), "jpeg_amd_transform_quanta")
    return out


def transform(source, op, region=None, requantize=None, threads: int = 0, path=None, ctx: Optional[Context] = None) -> bytes:
    """JPEG file -> JPEG file, losslessly rotated / flipped / cropped (and optionally requantised) in the coefficient domain
    (jpeg_amd_transform): the input's process, scan script, table keys, restart interval and metadata segments are kept.
    requantize: None or one table of 64 values per frame component, output orientation."""
    ctx = ctx or default_context()
    data = _file_bytes(source)
    reg = _region(region)
    rq = None
    if requantize is not None:
        rq = np.ascontiguousarray(np.stack([np.asarray(t, np.uint16).reshape(64) for t in requantize]))
    lib = _lib.lib()
    n = C.c_size_t()
    cap = 2 * data.size + (1 << 20)
    for _ in range(2):
        out = np.empty(cap, np.uint8)
        st = lib.jpeg_amd_transform(ctx.handle, data.ctypes.data, data.size, _xform_op(op), reg,
                                    rq.ctypes.data if rq is not None else None, int(threads), out.ctypes.data, out.size,
                                    C.byref(n), None)
        if st == _lib.EINVAL and n.value > cap:
            cap = n.value
            continue
        break
    _lib.check(st, "jpeg_amd_transform", ctx.handle)
    b = out[:n.value].tobytes()
    if path is not None:
        with open(path, "wb") as f:
            f.write(b)
    return b


def reduce_layout(size, layout: Layout, denom: int, units=None) -> Tuple[Tuple[int, int], List[Tuple[int, int]]]:
    """((W', H'), [(units_x, units_y) per plane]) of the image at 1/denom size as Spectral.reduce / reduce give it
    (jpeg_amd_reduce_layout): the units are recomputed from (W', H'), as a reader of the output file does."""
    L = layout.c_layout(size, units)
    out = _lib.Layout()
    _lib.check(_lib.lib().jpeg_amd_reduce_layout(C.byref(L), int(denom), C.byref(out)), "jpeg_amd_reduce_layout")
    return (out.width, out.height), [(out.units_x[p], out.units_y[p]) for p in range(layout.count)]


def reduce(source, denom: int, requantize=None, threads: int = 0, path=None, ctx: Optional[Context] = None) -> bytes:
    """JPEG file -> JPEG file at 1/denom size (denom 2 | 4 | 8) in the coefficient domain (jpeg_amd_reduce): the input's
    process, scan script, table keys, restart interval and metadata segments are kept.
    requantize: None (the file's own tables) or one output table of 64 values per frame component."""
    ctx = ctx or default_context()
    data = _file_bytes(source)
    rq = None
    if requantize is not None:
        rq = np.ascontiguousarray(np.stack([np.asarray(t, np.uint16).reshape(64) for t in requantize]))
    lib = _lib.lib()
    n = C.c_size_t()
    cap = 2 * data.size + (1 << 16)                  # one pass: a smaller image of the same script fits; else once more
    for _ in range(2):
        out = np.empty(cap, np.uint8)
        st = lib.jpeg_amd_reduce(ctx.handle, data.ctypes.data, data.size, int(denom), rq.ctypes.data if rq is not None else None,
                                 int(threads), out.ctypes.data, out.size, C.byref(n), None)
        if st == _lib.EINVAL and n.value > cap:
            cap = n.value
            continue
        break
    _lib.check(st, "jpeg_amd_reduce", ctx.handle)
    b = out[:n.value].tobytes()
    if path is not None:
        with open(path, "wb") as f:
            f.write(b)
    return b


def region_window(size, layout: Layout, region, cosite: bool = False, units=None) -> List[Tuple[int, int, int, int]]:
    """The block window (x, y, width, height in blocks) of every plane that the pixels of `region` read
    (jpeg_amd_region_window): what a caller uploads to decode that region."""
    L = layout.c_layout(size, units)
    w = (_lib.Region * MAX_PLANES)()
    _lib.check(_lib.lib().jpeg_amd_region_window(C.byref(L), 1 if cosite else 0, _region(region), w), "jpeg_amd_region_window")
    return [(w[p].x, w[p].y, w[p].width, w[p].height) for p in range(layout.count)]


def _batch_args(ctx: Context, size, layout: Layout, planes, quanta, q, n=None):
    """What the batch decodes of n images of one layout check and pass alike; n=None takes n from the planes.  -> (head, keep):
    the arguments between the context and `cosited` (layout, n, plane pointers and strides, tables, their stride and count),
    and the (n, planes, quanta on the device, c layout) that the pointers in `head` point into."""
    torch = _torch()
    q = list(q) if q is not None else _dedupe_q(layout)
    planes = list(planes)
    if len(planes) != layout.count or len(q) != layout.count:
        raise ValueError("plane count does not match layout")
    if n is None:
        n = int(planes[0].shape[0]) if planes and planes[0].dim() == 4 else -1
    for p in planes:
        if p.dtype != torch.int16 or not p.is_contiguous() or p.dim() != 4 or p.shape[0] != n:
            raise ValueError("planes: contiguous int16 device tensors [n, uy, ux, 64]")
    units = [(int(p.shape[2]), int(p.shape[1])) for p in planes]
    if isinstance(quanta, np.ndarray):
        quanta = ctx.upload(np.asarray(quanta, np.uint16))
    if quanta.dim() != 3 or quanta.shape[0] != n or quanta.shape[2] != 64 or not quanta.is_contiguous():
        raise ValueError("quanta: [n, ntables, 64]")
    L = layout.c_layout(size, units, q)
    ntables = int(quanta.shape[1])
    head = (C.byref(L), n, _ptrs(planes), _lib.size_array([p[0].numel() if n else 0 for p in planes]), quanta.data_ptr(),
            ntables * 64, ntables)
    return head, (n, planes, quanta, L)


def decode_regions(ctx: Context, size, layout: Layout, planes, quanta, regions, q: Optional[Sequence[int]] = None, color=RGB,
                   cosite: bool = False):
    """Decode n images of one layout, each cropped to its own region, in one call (jpeg_amd_decode_region_batch).
    planes[p]: device int16 [n, uy, ux, 64]; quanta: [n, ntables, 64] (host or device); regions: [n, 4] of (x, y, width,
    height) in pixels.  Returns n uint8 views [h_i, w_i, 3] into one allocation."""
    regs = np.ascontiguousarray(np.asarray(regions, np.int32).reshape(-1, 4))
    n = regs.shape[0]
    head, keep = _batch_args(ctx, size, layout, planes, quanta, q, n)
    areas = [3 * int(w) * int(h) for w, h in regs[:, 2:4]] if n else [0]
    stride = max(max(areas), 0)
    out = ctx.empty(n * stride, _torch().uint8)
    h_regions = (_lib.Region * max(n, 1))()
    for i, (x, y, w, h) in enumerate(regs.tolist()):
        h_regions[i].x, h_regions[i].y, h_regions[i].width, h_regions[i].height = x, y, w, h
    _lib.check(_lib.lib().jpeg_amd_decode_region_batch(ctx.handle, *head, 1 if cosite else 0, color.code, h_regions, out.data_ptr(),
                                                       stride), "jpeg_amd_decode_region_batch", ctx.handle)
    return [out[i * stride:i * stride + areas[i]].view(int(regs[i, 3]), int(regs[i, 2]), 3) for i in range(n)]


def scaled_size(size, denom: int) -> Tuple[int, int]:
    """(W', H') = (ceil(W N / 8), ceil(H N / 8)), N = 8 / denom: the size of a scaled decode (jpeg_amd_scaled_layout)."""
    if denom not in (1, 2, 4, 8):
        raise ValueError("denom: 1, 2, 4 or 8")
    n = 8 // denom
    return (int(size[0]) * n + 7) // 8, (int(size[1]) * n + 7) // 8


def decode_scaled(ctx: Context, size, layout: Layout, planes, quanta, denom: int, q: Optional[Sequence[int]] = None, color=RGB,
                  cosite: bool = False):
    """Decode n images of one layout at 1/denom size in one call (jpeg_amd_decode_scaled_batch).  planes[p]: device int16
    [n, uy, ux, 64]; quanta: [n, ntables, 64] (host or device).  Returns one uint8 tensor [n, H', W', 3]."""
    head, keep = _batch_args(ctx, size, layout, planes, quanta, q)
    n = keep[0]
    w, h = scaled_size(size, denom)
    stride = 3 * w * h
    out = ctx.empty(n * stride, _torch().uint8)
    _lib.check(_lib.lib().jpeg_amd_decode_scaled_batch(ctx.handle, *head, 1 if cosite else 0, color.code, int(denom), out.data_ptr(),
                                                       stride), "jpeg_amd_decode_scaled_batch", ctx.handle)
    return out.view(n, h, w, 3)


def view_window(size, layout: Layout, denom: int, region, cosite: bool = False, units=None) -> List[Tuple[int, int, int, int]]:
    """region_window for a view: the block window of every plane that the pixels of `region` of the image at 1/denom size
    read (jpeg_amd_view_window); of each block only the head of the scaled decode."""
    L = layout.c_layout(size, units)
    w = (_lib.Region * MAX_PLANES)()
    _lib.check(_lib.lib().jpeg_amd_view_window(C.byref(L), 1 if cosite else 0, int(denom), _region(region), w), "jpeg_amd_view_window")
    return [(w[p].x, w[p].y, w[p].width, w[p].height) for p in range(layout.count)]


def view_of_source(size, denom: int, source_region) -> Tuple[int, int, int, int]:
    """The smallest rectangle of the image at 1/denom size that covers `source_region`, a rectangle in pixels of the
    full-size image (jpeg_amd_view_of_source)."""
    L = _lib.Layout()
    L.width, L.height, L.precision, L.nplanes = int(size[0]), int(size[1]), 8, 1
    L.scale_x = L.scale_y = L.factor_x[0] = L.factor_y[0] = 1
    r = _lib.Region()
    _lib.check(_lib.lib().jpeg_amd_view_of_source(C.byref(L), int(denom), _region(source_region), C.byref(r)), "jpeg_amd_view_of_source")
    return r.x, r.y, r.width, r.height


def view_denom(source_size, want_size) -> int:
    """The largest denominator in (8, 4, 2, 1) at which a source rectangle of source_size (w, h) is still at least
    want_size (w, h): the cheapest view that needs no upscaling (jpeg_amd_view_denom)."""
    return int(_lib.lib().jpeg_amd_view_denom(int(source_size[0]), int(source_size[1]), int(want_size[0]), int(want_size[1])))


def _filter(filter) -> int:
    """filter="bilinear" | "antialias" | "bicubic" of the resample calls -> its JPEG_AMD_FILTER_* code."""
    codes = {"bilinear": _lib.FILTER_BILINEAR, "antialias": _lib.FILTER_ANTIALIAS, "bicubic": _lib.FILTER_BICUBIC}
    if filter not in codes:
        raise ValueError("filter: 'bilinear', 'antialias' or 'bicubic'")
    return codes[filter]


def _map_filter(filter) -> int:
    """filter="bilinear" | "bicubic" of the calls through a map ("bicubic warp": nothing is widened under a map, so no "antialias")."""
    codes = {"bilinear": _lib.FILTER_BILINEAR, "bicubic": _lib.FILTER_BICUBIC}
    if filter not in codes:
        raise ValueError("filter: 'bilinear' or 'bicubic' (a map has no 'antialias')")
    return codes[filter]


def _view_batch_args(ctx: Context, size, layout: Layout, planes, quanta, views, q):
    """The arguments decode_views, decode_resized and decode_tensors share: (vs [n, 5], head and keep of _batch_args, c views)."""
    vs, h_views = _views(views)
    head, keep = _batch_args(ctx, size, layout, planes, quanta, q, vs.shape[0])
    return vs, head, keep, h_views


def _views_out(ctx: Context, vs):
    """Room for the n views vs [n, 5] in one allocation -> (it, its stride, the n slices of it as uint8 [h_i, w_i, 3])."""
    n = vs.shape[0]
    areas = [3 * max(int(w), 0) * max(int(h), 0) for w, h in vs[:, 3:5]] if n else [0]
    stride = max(areas)
    out = ctx.empty(n * stride, _torch().uint8)
    return out, stride, [out[i * stride:i * stride + areas[i]].view(int(vs[i, 4]), int(vs[i, 3]), 3) for i in range(n)]


def decode_views(ctx: Context, size, layout: Layout, planes, quanta, views, q: Optional[Sequence[int]] = None, color=RGB,
                 cosite: bool = False):
    """Decode n images of one layout, each at its own denominator and cropped to its own rectangle of that scaled image, in
    one call (jpeg_amd_decode_view_batch).  planes[p]: device int16 [n, uy, ux, 64]; quanta: [n, ntables, 64] (host or
    device); views: [n, 5] of (denom, x, y, width, height).  Returns n uint8 views [h_i, w_i, 3] into one allocation."""
    vs, head, keep, h_views = _view_batch_args(ctx, size, layout, planes, quanta, views, q)
    out, stride, slices = _views_out(ctx, vs)
    _lib.check(_lib.lib().jpeg_amd_decode_view_batch(ctx.handle, *head, 1 if cosite else 0, color.code, h_views, out.data_ptr(), stride),
               "jpeg_amd_decode_view_batch", ctx.handle)
    return slices


def decode_resized(ctx: Context, size, layout: Layout, planes, quanta, views, out_size, q: Optional[Sequence[int]] = None,
                   color=RGB, cosite: bool = False, filter: str = "bilinear"):
    """decode_views with every image bilinearly resampled to out_size (Wt, Ht), in one call
    (jpeg_amd_decode_resized_filter_batch; include/jpeg_amd.h, "resized decode", holds the filter's contract).  Arguments as
    decode_views.  filter="antialias": the antialiasing filter instead ("antialiased resample" there), which refuses a view
    more than 16 times the target on an axis.  filter="bicubic": the Keys cubic (a = -0.5) widened by the scale factor
    ("bicubic resample" there; what torch's interpolate(mode="bicubic", antialias=True) computes, within one level), which
    refuses a view more than 8 times the target on an axis.  Returns one uint8 tensor [n, Ht, Wt, 3]."""
    code = _filter(filter)
    source = _view_batch_args(ctx, size, layout, planes, quanta, views, q)
    return _resample_batch(source, color, cosite, _Resample(ctx, source[0].shape[0], out_size, code).target())


def _crop_views(size, source_regions, out_size) -> np.ndarray:
    """The views of decode_crops_resized / decode_crops_tensor: int32 [n, 5] of (denom, x, y, width, height)."""
    regs = np.asarray(source_regions, np.int64).reshape(-1, 4)
    views = np.empty((regs.shape[0], 5), np.int32)
    for i, r in enumerate(regs.tolist()):
        denom = view_denom(r[2:], out_size)
        views[i] = (denom,) + view_of_source(size, denom, r)
    return views


def decode_crops_resized(ctx: Context, size, layout: Layout, planes, quanta, source_regions, out_size,
                         q: Optional[Sequence[int]] = None, color=RGB, cosite: bool = False, filter: str = "bilinear"):
    """The data-loader call: per image a rectangle (x, y, width, height) of the FULL-SIZE image, decoded at the cheapest
    denominator that is still no smaller than out_size -- view_denom((width, height), out_size), then view_of_source -- and
    resampled to out_size (Wt, Ht) by decode_resized, with its `filter` (the denominator is chosen the same way for every
    filter).  Returns (uint8 tensor [n, Ht, Wt, 3], the views it chose as int32
    [n, 5] of (denom, x, y, width, height))."""
    views = _crop_views(size, source_regions, out_size)
    return decode_resized(ctx, size, layout, planes, quanta, views, out_size, q=q, color=color, cosite=cosite, filter=filter), views


def _pack_images(ctx: Context, images):
    """Device uint8 images [h_i, w_i, 3] packed into one allocation (torch copies) -> (it, its stride, the extents)."""
    torch = _torch()
    n = len(images)
    for im in images:
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
            raise ValueError("images: uint8 device tensors [h, w, 3]")
    src_stride = max([int(im.numel()) for im in images] or [0])
    src = ctx.empty(n * src_stride, torch.uint8)
    extents = (_lib.Extent * max(n, 1))()
    for i, im in enumerate(images):
        src[i * src_stride:i * src_stride + im.numel()].copy_(im.reshape(-1))
        extents[i].width, extents[i].height = int(im.shape[1]), int(im.shape[0])
    return src, src_stride, extents


def resize(ctx: Context, images, out_size, filter: str = "bilinear", orientations=None, place=None, anchor="centre", fill=(0, 0, 0)):
    """Bilinearly resample n device uint8 images [h_i, w_i, 3] of any sizes to out_size (Wt, Ht) in one launch
    (jpeg_amd_resize_placed_batch), or with filter="antialias" through the antialiasing filter (no image more than 16 times
    the target on an axis), or with filter="bicubic" through the bicubic one (no image more than 8 times; decode_resized says
    which filter that is).  The images are packed into one allocation first (torch copies).  orientations: per image an EXIF
    orientation 1 .. 8 in which the image is read (include/jpeg_amd.h, "oriented resample").  place / anchor / fill: the image
    in a window of the out_size canvas and the fill's three bytes around it ("placed resample" there): place "fit" or "fit-down"
    (aspect-preserving, at `anchor` "centre" or "top-left") or one window (x, y, width, height) per image; with it the windows
    applied come back as an extra int32 [n, 4] item.  Returns uint8 [n, Ht, Wt, 3]."""
    code = _filter(filter)
    images = list(images)
    return _resample_images(images, _Resample(ctx, len(images), out_size, code).oriented(orientations).placed(place, anchor, fill))


def tensor_spec(mean=None, std=None, dtype=None, layout: str = "chw") -> _lib.TensorSpec:
    """The output stage of the tensor calls (struct jpeg_amd_tensor_spec) from the torchvision convention: mean and std per
    channel in 0 ... 1 units give mean_b = float32(255 mean) and scale = float32(1 / (255 std)), each computed in float64 and
    rounded once; element = (byte - mean_b) * scale.  mean=None: mean_b = 0; std=None: scale = 1 (both None: the bytes
    themselves as floats).  dtype: torch.float32, torch.float16 (the default) or torch.bfloat16; layout: "chw" or "hwc"."""
    torch = _torch()
    dtype = torch.float16 if dtype is None else dtype
    codes = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}
    layouts = {"hwc": _lib.TENSOR_HWC, "chw": _lib.TENSOR_CHW}
    if dtype not in codes or str(layout).lower() not in layouts:
        raise ValueError("tensor_spec: dtype float32 / float16 / bfloat16, layout 'chw' / 'hwc'")
    spec = _lib.TensorSpec()
    spec.dtype, spec.layout = codes[dtype], layouts[str(layout).lower()]
    for c in range(3):
        spec.mean[c] = 0.0 if mean is None else float(np.float32(255.0 * float(mean[c])))
        spec.scale[c] = 1.0 if std is None else float(np.float32(1.0 / (255.0 * float(std[c]))))
    return spec


class _Resample:
    """What a resample call was asked for, as one record (csrc/resample_request.hpp on this side).  A public function fills the
    columns in the order in which it judges its keyword arguments, the target (bytes or elements) last; the record keeps alive
    what the call points into, and a column the call does not carry is None, which the library takes as NULL."""

    def __init__(self, ctx: Context, n: int, out_size, code: int = _lib.FILTER_BILINEAR):
        self.ctx, self.n, self.out_size, self.code, self.k = ctx, n, out_size, code, 0   # k: the numbers of a matrix; 0: no map
        self.map_code, self.k_given = _lib.FILTER_BILINEAR, 0   # the filter of a map, and the numbers of a matrix as the caller gave it
        self.h_orient = self.placement = self.h_windows = self.tint = self.spec = self.h_flip = None

    def oriented(self, orientations, exif: bool = False):
        self.h_orient = _orientations(orientations, self.n, exif)
        return self

    def placed(self, place, anchor, fill):
        self.placement, self.h_windows, self._keep_windows = _placement(place, anchor, fill, self.n)
        return self

    def mapped(self, matrices, k: int, edge, fill, orientations=None, filter: str = "bilinear"):
        """k = 6: the affine map, 9: the homography.  The mixed calls judge their orientations behind the matrices.  filter:
        "bilinear", or "bicubic" ("bicubic warp"), which the projective calls alone carry: an affine map goes as the
        homography with the last row (0, 0, 1), and the matrices that come back are [n, 6] again (matrices_out)."""
        self.map_code = _map_filter(filter)
        self.k_given, m = k, _matrices(matrices, self.n, k)
        if self.map_code != _lib.FILTER_BILINEAR and k == 6:
            k, m = 9, _pad_affine(m)
        self.k, self.m, self.m_out = k, m, np.zeros((self.n, k), np.float32)
        if orientations is not None:
            self.oriented(orientations)
        self.warp = _warp(edge, fill)
        return self

    def matrices_out(self) -> np.ndarray:
        """The matrices a mixed or file call applied to its views, in the caller's form."""
        return self.m_out if self.k_given == self.k else np.ascontiguousarray(self.m_out[:, :self.k_given])

    def coloured(self, colour, colour_clamp):
        self.tint, self._keep_colour = _colour(colour, colour_clamp, self.n)
        return self

    def target(self, tensor=None):
        """The target, which comes last: room for n images of out_size, of bytes or with tensor = (spec, flips) of elements."""
        torch = _torch()
        self.wt, self.ht = int(self.out_size[0]), int(self.out_size[1])
        self.stride = 3 * max(self.wt, 0) * max(self.ht, 0)                 # between the images, in elements
        dtype = torch.uint8
        if tensor is not None:
            self.spec, flips = tensor
            dtype = {_lib.F32: torch.float32, _lib.F16: torch.float16, _lib.BF16: torch.bfloat16}.get(self.spec.dtype, torch.float32)
            if flips is not None:
                f = np.ascontiguousarray(np.asarray(flips).reshape(-1) != 0, np.uint8)
                if f.size != self.n:
                    raise ValueError("flips: one flag per image")
                self.h_flip = (C.c_uint8 * max(self.n, 1))(*f.tolist())
        self.out = self.ctx.empty(self.n * self.stride, dtype)
        return self

    def call(self, cells, head, lead=(), written=(), outputs=(), columns=True):
        """The one library call of the request: its cell (map x target) of a source's table, behind the source's `head`.  lead: the
        views or source rectangles, with a map the orientations; written: where a mixed call writes views and matrices."""
        target = () if self.spec is None else (C.byref(self.spec), self.h_flip)
        colour = () if self.spec is None else (None if self.tint is None else C.byref(self.tint),)
        if self.k:
            code = () if self.map_code == _lib.FILTER_BILINEAR else (self.map_code,)   # (the *_filter_* forms: behind the warp)
            args = lead + (self.m.ctypes.data, C.byref(self.warp)) + code + (self.wt, self.ht) + target + written + colour
        else:                                                # (the uniform batch has no columns)
            place = None if self.placement is None else C.byref(self.placement)
            args = lead + (self.wt, self.ht, self.code) + target + ((self.h_orient, place, self.h_windows) + colour if columns else ())
        name = cells[self.k, self.spec is not None]
        if self.k and self.map_code != _lib.FILTER_BILINEAR:
            name = _FILTER_CELLS[name]
        _lib.check(getattr(_lib.lib(), name)(self.ctx.handle, *head, *args, self.out.data_ptr(), self.stride, *outputs), name,
                   self.ctx.handle)

    def result(self, *written):
        """The output tensor, then `written`, then with a placement the windows applied; one item comes back bare."""
        chw = self.spec is not None and self.spec.layout == _lib.TENSOR_CHW
        out = self.out.view(self.n, 3, self.ht, self.wt) if chw else self.out.view(self.n, self.ht, self.wt, 3)
        if self.placement is not None:
            written += (np.array([(r.x, r.y, r.width, r.height) for r in self.h_windows[:self.n]], np.int32).reshape(self.n, 4),)
        return (out,) + written if written else out


# The widest entry point of every cell, source by source: (numbers of a matrix, tensor target) -> symbol (csrc/capi_*.hip).
_BATCH_CELLS = {(0, False): "jpeg_amd_decode_resized_filter_batch", (0, True): "jpeg_amd_decode_tensor_filter_batch"}
_IMAGE_CELLS = {(0, False): "jpeg_amd_resize_placed_batch", (0, True): "jpeg_amd_resize_colour_tensor_batch",
                (6, False): "jpeg_amd_warp_batch", (6, True): "jpeg_amd_warp_colour_tensor_batch",
                (9, False): "jpeg_amd_project_batch", (9, True): "jpeg_amd_project_tensor_batch"}
_MIXED_CELLS = {(0, False): "jpeg_amd_decode_resized_placed_mixed", (0, True): "jpeg_amd_decode_tensor_colour_mixed",
                (6, False): "jpeg_amd_decode_warped_mixed", (6, True): "jpeg_amd_decode_tensor_warped_colour_mixed",
                (9, False): "jpeg_amd_decode_projected_mixed", (9, True): "jpeg_amd_decode_tensor_projected_mixed"}
_FILE_CELLS = {(0, False): "jpeg_amd_decompress_resized_placed_mixed", (0, True): "jpeg_amd_decompress_tensor_colour_mixed",
               (6, False): "jpeg_amd_decompress_resized_warped_mixed", (6, True): "jpeg_amd_decompress_tensor_warped_colour_mixed",
               (9, False): "jpeg_amd_decompress_resized_projected_mixed", (9, True): "jpeg_amd_decompress_tensor_projected_mixed"}


# ... and of the projective cells the form with a filter ("bicubic warp"), which a map with another filter than the bilinear takes.
_FILTER_CELLS = {"jpeg_amd_project_batch": "jpeg_amd_project_filter_batch",
                 "jpeg_amd_project_tensor_batch": "jpeg_amd_project_filter_tensor_batch",
                 "jpeg_amd_decode_projected_mixed": "jpeg_amd_decode_projected_filter_mixed",
                 "jpeg_amd_decode_tensor_projected_mixed": "jpeg_amd_decode_tensor_projected_filter_mixed",
                 "jpeg_amd_decompress_resized_projected_mixed": "jpeg_amd_decompress_resized_projected_filter_mixed",
                 "jpeg_amd_decompress_tensor_projected_mixed": "jpeg_amd_decompress_tensor_projected_filter_mixed"}


def _resample_batch(source, color, cosite: bool, rq: _Resample):
    """The route of the uniform batch; source: what _view_batch_args returns."""
    vs, head, keep, h_views = source
    rq.call(_BATCH_CELLS, head + (1 if cosite else 0, color.code, h_views), columns=False)
    return rq.result()


def _resample_images(images, rq: _Resample, tensor=None):
    """The route of device images, which are packed here, behind the request's other complaints and in front of its target's."""
    src, src_stride, extents = _pack_images(rq.ctx, images)
    rq.target(tensor).call(_IMAGE_CELLS, (rq.n, src.data_ptr(), src_stride, extents))
    return rq.result()


def _resample_mixed(source, color, cosite: bool, rq: _Resample):
    """The route of Spectral images of mixed layouts; source: what _mixed_args returns (with a map: of placeholder views)."""
    vs, h_images, h_views, keep = source
    lead, written = ((rq.h_orient,), (h_views, rq.m_out.ctypes.data)) if rq.k else ((h_views,), ())
    rq.call(_MIXED_CELLS, (rq.n, h_images, 1 if cosite else 0, color.code), lead, written)
    return rq.result(_views_array(h_views, rq.n), rq.matrices_out()) if rq.k else rq.result()


def _resample_files(source, threads: int, color, cosite: bool, rq: _Resample):
    """The route of files; source: what _file_args returns.  -> the orientations applied: the wide forms always have room."""
    n, ptrs, sizes, regions, infos, h_views, keep = source
    head = (ptrs, sizes, n, int(threads), 1 if cosite else 0, color.code)
    applied = (C.c_int32 * max(n, 1))()
    lead, matrices = ((rq.h_orient,), (rq.m_out.ctypes.data,)) if rq.k else ((regions,), ())
    rq.call(_FILE_CELLS, head, lead, outputs=(infos, h_views) + matrices + (applied,))
    return np.array(applied[:n], np.int32)


def decode_tensors(ctx: Context, size, layout: Layout, planes, quanta, views, out_size, spec: _lib.TensorSpec, flips=None,
                   q: Optional[Sequence[int]] = None, color=RGB, cosite: bool = False, filter: str = "bilinear"):
    """decode_resized with the loader's tail in the same call (jpeg_amd_decode_tensor_filter_batch; include/jpeg_amd.h,
    "tensor output", holds the contract): every view resampled to out_size (Wt, Ht), mirrored along x where flips[i] is set,
    normalised by `spec` (tensor_spec) and stored in its dtype and layout; `filter` as in decode_resized.  Returns one tensor
    [n, 3, Ht, Wt] ("chw") or [n, Ht, Wt, 3] ("hwc")."""
    code = _filter(filter)
    source = _view_batch_args(ctx, size, layout, planes, quanta, views, q)
    return _resample_batch(source, color, cosite, _Resample(ctx, source[0].shape[0], out_size, code).target((spec, flips)))


def decode_crops_tensor(ctx: Context, size, layout: Layout, planes, quanta, source_regions, out_size, spec: _lib.TensorSpec,
                        flips=None, q: Optional[Sequence[int]] = None, color=RGB, cosite: bool = False, filter: str = "bilinear"):
    """The data-loader call, to the tensor a training loop takes: the views decode_crops_resized chooses for the rectangles
    (x, y, width, height) of the FULL-SIZE images, through decode_tensors with its `filter`.  Returns (tensor, the views as int32 [n, 5])."""
    views = _crop_views(size, source_regions, out_size)
    return decode_tensors(ctx, size, layout, planes, quanta, views, out_size, spec, flips=flips, q=q, color=color, cosite=cosite,
                          filter=filter), views


def _mixed_args(ctx: Context, spectrals, views):
    """The arguments the mixed calls share: (vs [n, 5], c images, c views, keep).  Every image's tables go up in ONE upload;
    `keep` holds what the pointers in the c images point into."""
    torch = _torch()
    spectrals = list(spectrals)
    vs, h_views = _views(views)
    n = vs.shape[0]
    if len(spectrals) != n:
        raise ValueError("views: one (denom, x, y, width, height) per image")
    tables = [t for s in spectrals for t in s.quanta]
    quanta = ctx.upload(np.stack(tables).astype(np.uint16)) if tables else None
    h_images = (_lib.Image * max(n, 1))()
    first = 0
    for i, s in enumerate(spectrals):
        for p in s.planes:
            if p.dtype != torch.int16 or not p.is_contiguous():
                raise ValueError("spectrals: planes are contiguous int16 device tensors")
        h_images[i].layout = s._layout()
        for p, plane in enumerate(s.planes):
            h_images[i].d_coef[p] = plane.data_ptr()
        h_images[i].d_quanta = quanta.data_ptr() + 128 * first
        h_images[i].ntables = len(s.quanta)
        first += len(s.quanta)
    return vs, h_images, h_views, (spectrals, quanta)


def decode_views_mixed(ctx: Context, spectrals, views, color=RGB, cosite: bool = False):
    """decode_views for images of DIFFERENT sizes and layouts in one call (jpeg_amd_decode_view_mixed).  spectrals: a sequence
    of Spectral objects (what Spectral.decompress returns), any mix of sizes, of 4:4:4 / 4:2:2 / 4:4:0 / 4:2:0 and of grey;
    views: [n, 5] of (denom, x, y, width, height), each against its own image.  Image i is what Spectral.view gives for it.
    Returns n uint8 views [h_i, w_i, 3] into one allocation."""
    vs, h_images, h_views, keep = _mixed_args(ctx, spectrals, views)
    out, stride, slices = _views_out(ctx, vs)
    _lib.check(_lib.lib().jpeg_amd_decode_view_mixed(ctx.handle, vs.shape[0], h_images, 1 if cosite else 0, color.code, h_views,
                                                     out.data_ptr(), stride), "jpeg_amd_decode_view_mixed", ctx.handle)
    return slices


def decode_resized_mixed(ctx: Context, spectrals, views, out_size, color=RGB, cosite: bool = False, filter: str = "bilinear",
                         orientations=None, place=None, anchor="centre", fill=(0, 0, 0)):
    """decode_resized for images of different sizes and layouts in one call (jpeg_amd_decode_resized_placed_mixed);
    arguments as decode_views_mixed, `filter` as in decode_resized.  orientations: per image an EXIF orientation 1 .. 8 in which
    its view's pixels are read; the views stay rectangles of the STORED scaled images.  place / anchor / fill: as in resize;
    "fit" fits the oriented view.  Returns one uint8 tensor [n, Ht, Wt, 3]."""
    code = _filter(filter)
    source = _mixed_args(ctx, spectrals, views)
    rq = _Resample(ctx, source[0].shape[0], out_size, code).oriented(orientations).placed(place, anchor, fill)
    return _resample_mixed(source, color, cosite, rq.target())


def decode_tensors_mixed(ctx: Context, spectrals, views, out_size, spec: _lib.TensorSpec, flips=None, color=RGB,
                         cosite: bool = False, filter: str = "bilinear", orientations=None, place=None, anchor="centre",
                         fill=(0, 0, 0), colour=None, colour_clamp=None):
    """decode_tensors for images of different sizes and layouts in one call (jpeg_amd_decode_tensor_colour_mixed); arguments
    as decode_views_mixed, then as decode_tensors, `filter` ("bilinear" | "antialias" | "bicubic") included.  orientations: as
    in decode_resized_mixed; a flip mirrors the output after the orientation.  place / anchor / fill: as in resize; a flip
    mirrors the whole canvas.  colour / colour_clamp: as in resize_tensor.
    Returns one tensor [n, 3, Ht, Wt] ("chw") or [n, Ht, Wt, 3] ("hwc")."""
    code = _filter(filter)
    source = _mixed_args(ctx, spectrals, views)
    rq = _Resample(ctx, source[0].shape[0], out_size, code).oriented(orientations).placed(place, anchor, fill)
    return _resample_mixed(source, color, cosite, rq.coloured(colour, colour_clamp).target((spec, flips)))


def decode_crops_tensor_mixed(ctx: Context, spectrals, source_regions, out_size, spec: _lib.TensorSpec, flips=None, color=RGB,
                              cosite: bool = False, filter: str = "bilinear", orientations=None, place=None, anchor="centre",
                              fill=(0, 0, 0), colour=None, colour_clamp=None):
    """The data-loader call over files of different sizes and layouts: per image a rectangle (x, y, width, height) of ITS
    full-size image, the view chosen as decode_crops_tensor chooses it -- view_denom, then view_of_source on that image's own
    size -- through decode_tensors_mixed, with its `filter`.  orientations: per image an EXIF orientation 1 .. 8; the rectangles are then
    rectangles of the ORIENTED images: the denominator is chosen for the oriented rectangle and the view is that of the stored
    rectangle orient_region maps it to.  place / anchor / fill: as in resize; "fit" fits the (oriented) rectangle, and the
    denominator is chosen against the window, not the canvas.  colour / colour_clamp: as in decode_tensors_mixed.
    Returns (tensor, the views as int32 [n, 5]: stored scaled coordinates), and with `place` the windows as int32 [n, 4]."""
    spectrals = list(spectrals)
    regs = np.asarray(source_regions, np.int64).reshape(-1, 4)
    if regs.shape[0] != len(spectrals):
        raise ValueError("source_regions: one (x, y, width, height) per image")
    orientations = None if orientations is None else list(orientations)
    if orientations is not None and len(orientations) != len(spectrals):
        raise ValueError("orientations: one value in 1 .. 8 per image")
    views = np.empty((len(spectrals), 5), np.int32)
    windows = None
    if place is not None:
        if isinstance(place, str):
            place = [place_window(place, regs[i, 2:], out_size, anchor) for i in range(len(spectrals))]
        windows = np.asarray(place, np.int64).reshape(-1, 4)
        if windows.shape[0] != len(spectrals):
            raise ValueError("place: one (x, y, width, height) per image")
    for i, s in enumerate(spectrals):
        denom = view_denom(regs[i, 2:], out_size if windows is None else windows[i, 2:])
        stored = regs[i].tolist() if orientations is None else orient_region(orientations[i], s.size, regs[i].tolist())
        views[i] = (denom,) + view_of_source(s.size, denom, stored)
    res = decode_tensors_mixed(ctx, spectrals, views, out_size, spec, flips=flips, color=color, cosite=cosite, filter=filter,
                               orientations=orientations, place=windows, anchor=anchor, fill=fill, colour=colour, colour_clamp=colour_clamp)
    return (res, views) if windows is None else (res[0], views, res[1])


def _resample_mapped(ctx: Context, sources, matrices, k: int, out_size, edge, fill, tensor=None, mixed=None, filter: str = "bilinear"):
    """The warp (k = 6) and project (k = 9) calls of device images, or with mixed = (color, cosite, orientations) of Spectral
    images.  tensor: None for bytes, or the (spec, flips, colour, colour_clamp) of the tensor forms.  filter: of the map."""
    _map_filter(filter)
    sources = list(sources)
    source = mixed and _mixed_args(ctx, sources, np.zeros((len(sources), 5), np.int32))   # (placeholder views: the call writes them)
    rq = _Resample(ctx, len(sources), out_size).mapped(matrices, k, edge, fill, mixed and mixed[2], filter)
    if tensor:
        rq.coloured(*tensor[2:])
    if not mixed:
        return _resample_images(sources, rq, tensor and tensor[:2])
    return _resample_mixed(source, mixed[0], mixed[1], rq.target(tensor and tensor[:2]))


def decode_warped_mixed(ctx: Context, spectrals, matrices, out_size, color=RGB, cosite: bool = False, orientations=None,
                        edge="fill", fill=(0, 0, 0), filter: str = "bilinear"):
    """The warp from Spectral images of different sizes and layouts in one call (jpeg_amd_decode_warped_mixed; include/jpeg_amd.h,
    "warped resample"): per image a matrix [6] in the coordinates of its UPRIGHT full-size image (the stored image seen through
    orientations[i], 1 .. 8; None: as stored).  warp_view chooses each image's denominator and view -- only the part the canvas
    maps into is decoded -- and image i is warp() of decode_views_mixed's pixels for that view with the matrix against it.
    filter: "bilinear" or "bicubic", as in warp; the views are warp_view's with that filter.
    Returns (uint8 [n, Ht, Wt, 3], the views as int32 [n, 5], the matrices applied to them as float32 [n, 6])."""
    return _resample_mapped(ctx, spectrals, matrices, 6, out_size, edge, fill, None, (color, cosite, orientations), filter)


def decode_tensors_warped_mixed(ctx: Context, spectrals, matrices, out_size, spec: _lib.TensorSpec, flips=None, color=RGB,
                                cosite: bool = False, orientations=None, edge="fill", fill=(0, 0, 0), colour=None, colour_clamp=None,
                                filter: str = "bilinear"):
    """decode_warped_mixed with the output stage of the tensor calls (jpeg_amd_decode_tensor_warped_colour_mixed); flips, spec,
    colour and colour_clamp as in warp_tensor, filter as in decode_warped_mixed.
    Returns (tensor [n, 3, Ht, Wt] or [n, Ht, Wt, 3], the views as int32 [n, 5], the matrices as float32 [n, 6])."""
    return _resample_mapped(ctx, spectrals, matrices, 6, out_size, edge, fill, (spec, flips, colour, colour_clamp),
                            (color, cosite, orientations), filter)


def decode_projected_mixed(ctx: Context, spectrals, matrices, out_size, color=RGB, cosite: bool = False, orientations=None,
                           edge="fill", fill=(0, 0, 0), filter: str = "bilinear"):
    """decode_warped_mixed through a 3 x 3 homography per image (jpeg_amd_decode_projected_mixed; include/jpeg_amd.h,
    "projective resample"): matrices [n, 9] or [n, 3, 3] in the coordinates of the UPRIGHT full-size images (perspective_matrix
    makes one from four point pairs).  project_view chooses each image's denominator and view, and image i is project() of
    decode_views_mixed's pixels for that view with the matrix against it.  filter: "bilinear" or "bicubic", as in project
    (jpeg_amd_decode_projected_filter_mixed; the views are project_view's with that filter).
    Returns (uint8 [n, Ht, Wt, 3], the views as int32 [n, 5], the matrices applied to them as float32 [n, 9])."""
    return _resample_mapped(ctx, spectrals, matrices, 9, out_size, edge, fill, None, (color, cosite, orientations), filter)


def decode_tensors_projected_mixed(ctx: Context, spectrals, matrices, out_size, spec: _lib.TensorSpec, flips=None, color=RGB,
                                   cosite: bool = False, orientations=None, edge="fill", fill=(0, 0, 0), colour=None,
                                   colour_clamp=None, filter: str = "bilinear"):
    """decode_projected_mixed with the output stage of the tensor calls (jpeg_amd_decode_tensor_projected_mixed); flips, spec,
    colour and colour_clamp as in project_tensor, filter as in decode_projected_mixed.
    Returns (tensor [n, 3, Ht, Wt] or [n, Ht, Wt, 3], the views as int32 [n, 5], the matrices as float32 [n, 9])."""
    return _resample_mapped(ctx, spectrals, matrices, 9, out_size, edge, fill, (spec, flips, colour, colour_clamp),
                            (color, cosite, orientations), filter)


def _file_args(sources, source_regions):
    """The arguments the file calls share: (n, c file pointers, c sizes, c source rectangles or None, room for the frame
    infos, room for the views, keep).  sources: paths or the files' bytes."""
    files = [_file_bytes(s) for s in sources]
    n = len(files)
    ptrs = (C.c_void_p * max(n, 1))(*[f.ctypes.data for f in files])
    sizes = (C.c_size_t * max(n, 1))(*[f.size for f in files])
    regions = None
    if source_regions is not None:
        regs = np.asarray(source_regions, np.int64).reshape(-1, 4)
        if regs.shape[0] != n:
            raise ValueError("source_regions: one (x, y, width, height) per file")
        regions = (_lib.Region * max(n, 1))()
        for i, r in enumerate(regs.tolist()):
            regions[i].x, regions[i].y, regions[i].width, regions[i].height = r
    return n, ptrs, sizes, regions, (_lib.FrameInfo * max(n, 1))(), (_lib.View * max(n, 1))(), files


def _file_columns(rq: _Resample, warp, edge, source_regions, place, anchor, fill, warp_filter=None) -> _Resample:
    """warp=, edge=, fill=, warp_filter= of the file calls, or without a warp their place=, anchor=, fill=."""
    if warp is None:
        if warp_filter is not None:
            raise ValueError("warp_filter: only together with warp")
        return rq.placed(place, anchor, fill)
    if source_regions is not None or place is not None or rq.code != _lib.FILTER_BILINEAR:
        raise ValueError('warp: not together with source_regions, place or a filter other than "bilinear"')
    shape = np.shape(warp)                                   # [n, 9] or [n, 3, 3]: the homography; else the affine map [n, 6]
    return rq.mapped(warp, 9 if shape[-1:] == (9,) or shape[-2:] == (3, 3) else 6, edge, fill,
                     filter="bilinear" if warp_filter is None else warp_filter)


def _views_array(h_views, n) -> np.ndarray:
    return np.array([(v.denom, v.region.x, v.region.y, v.region.width, v.region.height) for v in h_views[:n]], np.int32).reshape(n, 5)


def decompress_tensors(ctx: Context, sources, out_size, spec: _lib.TensorSpec, source_regions=None, flips=None, color=RGB,
                       cosite: bool = False, filter: str = "bilinear", threads: int = 0, orientation=None, place=None,
                       anchor="centre", fill=(0, 0, 0), warp=None, edge="fill", colour=None, colour_clamp=None, warp_filter=None):
    """The data-loader call from FILES: n JPEG files (paths or bytes) of any mix of sizes, of 4:4:4 / 4:2:2 / 4:4:0 / 4:2:0, grey
    and progressive, to one normalised tensor in one call (jpeg_amd_decompress_tensor_colour_mixed, with `warp`
    jpeg_amd_decompress_tensor_warped_colour_mixed or jpeg_amd_decompress_tensor_projected_mixed; include/jpeg_amd.h, "files to
    tensors").  Image i is what decode_crops_tensor_mixed gives for Spectral.decompress of file i: per file a rectangle
    (x, y, width, height) of its full-size image (source_regions; None: the whole images), decoded at the cheapest denominator
    that is still no smaller than out_size (Wt, Ht), resampled by `filter` ("bilinear" | "antialias" | "bicubic", as in
    decode_resized), mirrored where flips[i] is set, normalised by `spec` (tensor_spec).  The files are entropy-decoded on
    `threads` host threads (0: all cores) into the sparse form, and only the parts of the coefficient planes that the views read
    are rebuilt on the device.
    orientation: None (the images as they are stored), "exif" (every file in the orientation its EXIF segment names:
    exif_orientation) or a sequence of 1 .. 8 or "exif" per file ("oriented resample" there).  With it, source_regions are
    rectangles of the ORIENTED images -- the images a viewer shows -- while the views that come back stay in stored scaled
    coordinates.
    Returns (tensor [n, 3, Ht, Wt] or [n, Ht, Wt, 3], the views as int32 [n, 5] of (denom, x, y, width, height), the files'
    frame infos), and with `orientation` given a fourth item, the orientations applied as int32 [n].
    place / anchor / fill: as in resize; "fit" fits the (oriented) source rectangle, and the denominator is chosen against the
    window; with `place` the windows applied come back as the last item.
    warp / edge / fill: per file a matrix [6] in the coordinates of its UPRIGHT full-size image, as in decode_warped_mixed
    ("warped resample" there); not together with source_regions, place or a filter other than "bilinear" (ValueError).  The
    views that come back are warp_view's, and the matrices applied to them come back as the last item, float32 [n, 6].  A warp
    of [n, 9] or [n, 3, 3] is a homography per file ("projective resample"): the views are project_view's and the matrices that
    come back float32 [n, 9].  warp_filter: the filter of the warp, "bilinear" (None) or "bicubic" as in warp ("bicubic warp";
    the views are then one pixel wider on each side); only together with `warp` (ValueError).  `filter` is the resize's and
    stays "bilinear" with a warp.
    colour / colour_clamp: as in resize_tensor, per file; what comes back is what the call without them returns."""
    code = _filter(filter)
    source = _file_args(sources, source_regions)
    n, infos, h_views = source[0], source[4], source[5]
    rq = _Resample(ctx, n, out_size, code).oriented(orientation, exif=True).coloured(colour, colour_clamp)
    rq = _file_columns(rq, warp, edge, source_regions, place, anchor, fill, warp_filter).target((spec, flips))
    applied = _resample_files(source, threads, color, cosite, rq)
    written = (_views_array(h_views, n), list(infos[:n])) + (() if rq.h_orient is None else (applied,))
    return rq.result(*written, *((rq.matrices_out(),) if rq.k else ()))


def decompress_resized(ctx: Context, sources, out_size, source_regions=None, color=RGB, cosite: bool = False,
                       filter: str = "bilinear", threads: int = 0, orientation=None, place=None, anchor="centre", fill=(0, 0, 0),
                       warp=None, edge="fill", warp_filter=None):
    """decompress_tensors without the tensor stage (jpeg_amd_decompress_resized_placed_mixed, with `warp`
    jpeg_amd_decompress_resized_warped_mixed or jpeg_amd_decompress_resized_projected_mixed): the files' views resampled to
    out_size (Wt, Ht) as bytes by `filter`; `orientation` as there.  place / anchor / fill: as there, the windows as a second
    item.  warp / edge / fill: as there; with it the views (int32 [n, 5]) and the matrices applied to them (float32 [n, 6]; of a
    [n, 9] or [n, 3, 3] warp [n, 9]) come back as the last two items; warp_filter: as there.
    Returns one uint8 tensor [n, Ht, Wt, 3]."""
    code = _filter(filter)
    source = _file_args(sources, source_regions)
    rq = _Resample(ctx, source[0], out_size, code).oriented(orientation, exif=True)
    rq = _file_columns(rq, warp, edge, source_regions, place, anchor, fill, warp_filter).target()
    _resample_files(source, threads, color, cosite, rq)
    return rq.result(_views_array(source[5], rq.n), rq.matrices_out()) if rq.k else rq.result()


def resize_tensor(ctx: Context, images, out_size, spec: _lib.TensorSpec, flips=None, filter: str = "bilinear", orientations=None,
                  place=None, anchor="centre", fill=(0, 0, 0), colour=None, colour_clamp=None):
    """The resample and the output stage alone (jpeg_amd_resize_colour_tensor_batch; `filter` as in resize): n device uint8
    images [h_i, w_i, 3] of any sizes to one tensor [n, 3, Ht, Wt] or [n, Ht, Wt, 3] of spec's dtype, in one launch.
    orientations: as in resize; a flip mirrors the output after the orientation.  place / anchor / fill: as in resize; a padded
    element is the fill byte through `spec`, and a flip mirrors the whole canvas, window position included.
    colour / colour_clamp: per image a matrix [3, 4] (colour_matrix makes one; [n, 3, 4] or [n, 12]) applied to every pixel's
    (R, G, B), fill pixels included, in front of spec's mean, then clamped to colour_clamp = (lo, hi) in byte units (None: no
    clamp), in the same launch (include/jpeg_amd.h, "colour stage")."""
    code = _filter(filter)
    images = list(images)
    rq = _Resample(ctx, len(images), out_size, code).oriented(orientations).placed(place, anchor, fill).coloured(colour, colour_clamp)
    return _resample_images(images, rq, (spec, flips))


def warp(ctx: Context, images, matrices, out_size, edge="fill", fill=(0, 0, 0), filter: str = "bilinear"):
    """n device uint8 images [h_i, w_i, 3] of any sizes through an affine map each, to out_size (Wt, Ht), in one launch
    (jpeg_amd_warp_batch; include/jpeg_amd.h, "warped resample", holds the contract).  matrices: [n, 6] of (m00, m01, m02, m10,
    m11, m12), the INVERSE map from the centres of output pixels to source coordinates (affine_matrix makes one from an angle,
    a scale and a shear).  edge: "fill" (a tap outside the image has the `fill` bytes: grid_sample's "zeros") or "replicate"
    (its index is clamped: "border").  filter: "bilinear", or "bicubic" (include/jpeg_amd.h, "bicubic warp": 4 x 4 fixed taps
    of the Keys cubic with a = -0.5, PIL's BICUBIC under a rotation; through jpeg_amd_project_filter_batch with the last row
    (0, 0, 1)); "antialias" is a ValueError: nothing is widened under a map.  Returns uint8 [n, Ht, Wt, 3]."""
    return _resample_mapped(ctx, images, matrices, 6, out_size, edge, fill, filter=filter)


def warp_tensor(ctx: Context, images, matrices, out_size, spec: _lib.TensorSpec, flips=None, edge="fill", fill=(0, 0, 0),
                colour=None, colour_clamp=None, filter: str = "bilinear"):
    """warp with the output stage of the tensor calls (jpeg_amd_warp_colour_tensor_batch): the warped image mirrored along x
    where flips[i] is set, normalised by `spec` (fill pixels included) and stored in its dtype and layout.  colour /
    colour_clamp: as in resize_tensor; filter: as in warp.  Returns one tensor [n, 3, Ht, Wt] ("chw") or [n, Ht, Wt, 3] ("hwc")."""
    return _resample_mapped(ctx, images, matrices, 6, out_size, edge, fill, (spec, flips, colour, colour_clamp), filter=filter)


def project(ctx: Context, images, matrices, out_size, edge="fill", fill=(0, 0, 0), filter: str = "bilinear"):
    """warp through a 3 x 3 homography per image (jpeg_amd_project_batch; include/jpeg_amd.h, "projective resample", holds the
    contract): matrices [n, 9] or [n, 3, 3], row by row, the INVERSE projective map from the centres of output pixels to source
    coordinates (perspective_matrix makes one from four point pairs).  The denominator m20 x + m21 y + m22 must stay positive
    and within 16 : 1 over the canvas (the library judges it).  With the last row (0, 0, 1) this is warp on the first six
    numbers, bit for bit.  filter: "bilinear" or "bicubic", as in warp (jpeg_amd_project_filter_batch).
    Returns uint8 [n, Ht, Wt, 3]."""
    return _resample_mapped(ctx, images, matrices, 9, out_size, edge, fill, filter=filter)


def project_tensor(ctx: Context, images, matrices, out_size, spec: _lib.TensorSpec, flips=None, edge="fill", fill=(0, 0, 0),
                   colour=None, colour_clamp=None, filter: str = "bilinear"):
    """project with the output stage of the tensor calls (jpeg_amd_project_tensor_batch): flips, spec, colour and colour_clamp
    as in warp_tensor, filter as in project.  Returns one tensor [n, 3, Ht, Wt] ("chw") or [n, Ht, Wt, 3] ("hwc")."""
    return _resample_mapped(ctx, images, matrices, 9, out_size, edge, fill, (spec, flips, colour, colour_clamp), filter=filter)


def tensor_source(mean=None, std=None, dtype=None, layout: str = "chw") -> _lib.TensorSource:
    """The input stage of the tensor encode calls (struct jpeg_amd_tensor_source), the inverse of tensor_spec: mean and std per
    channel in 0 ... 1 units give scale = float32(255 std) and offset = float32(255 mean), each computed in float64 and rounded
    once; byte = clamp(element * scale + offset) rounded.  std=None: scale = 1; mean=None: offset = 0 (both None: elements
    in byte units; std (1, 1, 1) and mean (0, 0, 0): elements in 0 ... 1).  dtype: torch.float32, torch.float16 (the default),
    torch.bfloat16 or torch.uint8 (the bytes themselves; mean and std are not used); layout: "chw" or "hwc"."""
    torch = _torch()
    dtype = torch.float16 if dtype is None else dtype
    codes = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16, torch.uint8: _lib.U8}
    layouts = {"hwc": _lib.TENSOR_HWC, "chw": _lib.TENSOR_CHW}
    if dtype not in codes or str(layout).lower() not in layouts:
        raise ValueError("tensor_source: dtype float32 / float16 / bfloat16 / uint8, layout 'chw' / 'hwc'")
    src = _lib.TensorSource()
    src.dtype, src.layout = codes[dtype], layouts[str(layout).lower()]
    for c in range(3):
        src.scale[c] = 1.0 if std is None else float(np.float32(255.0 * float(std[c])))
        src.offset[c] = 0.0 if mean is None else float(np.float32(255.0 * float(mean[c])))
    return src


def _source_args(ctx: Context, tensors, source: _lib.TensorSource):
    """What the tensor encode calls take of `tensors`, [n, 3, H, W] ("chw") or [n, H, W, 3] ("hwc") of source's dtype on the
    context's device, each image contiguous: -> (n, W, H, elements between the images)."""
    torch = _torch()
    dtypes = {_lib.F32: torch.float32, _lib.F16: torch.float16, _lib.BF16: torch.bfloat16, _lib.U8: torch.uint8}
    if not isinstance(tensors, torch.Tensor) or tensors.dim() != 4:
        raise ValueError("tensors: one tensor [n, 3, H, W] or [n, H, W, 3]")
    if tensors.dtype != dtypes.get(source.dtype):
        raise ValueError("tensors: dtype %s does not match the source's" % tensors.dtype)
    n = int(tensors.shape[0])
    c, h, w = tensors.shape[1:] if source.layout == _lib.TENSOR_CHW else (tensors.shape[3], tensors.shape[1], tensors.shape[2])
    if c != 3 or h < 1 or w < 1:
        raise ValueError("tensors: three channels in the source's layout, H and W at least 1")
    if tensors.device != ctx.torch_device:
        raise ValueError("tensors: on the context's device")
    if n > 0 and not tensors[0].is_contiguous():
        raise ValueError("tensors: each image contiguous")
    stride = int(tensors.stride(0)) if n > 1 else 3 * int(w) * int(h)
    if stride < 3 * w * h:
        raise ValueError("tensors: images overlap")
    return n, int(w), int(h), stride


def _encode_tables(layout: Layout, quanta):
    """-> (one table per distinct quanta key of the layout in plane order, the table index of every plane)."""
    q = _dedupe_q(layout)
    keys: List[int] = []
    for c in layout.planes:
        if c.qi not in quanta:
            raise _lib.JpegAmdError(_lib.EINVAL, f"missing quantization table for quanta key {c.qi}")
        if c.qi not in keys:
            keys.append(c.qi)
    return [np.asarray(quanta[k], np.uint16).reshape(64) for k in keys], q


def tensor_pixels(ctx: Context, tensors, source: _lib.TensorSource):
    """Tensors to the encoders' bytes in one launch (jpeg_amd_tensor_pixels_batch; include/jpeg_amd.h, "tensor sources", holds
    the contract).  tensors: [n, 3, H, W] or [n, H, W, 3] as `source` (tensor_source) says, on the context's device, each image
    contiguous, the batch stride taken from stride(0).  Returns uint8 [n, H, W, 3]."""
    n, w, h, stride = _source_args(ctx, tensors, source)
    out = ctx.empty(n * 3 * w * h, _torch().uint8)
    _lib.check(_lib.lib().jpeg_amd_tensor_pixels_batch(ctx.handle, n, tensors.data_ptr(), stride, w, h, C.byref(source),
                                                       out.data_ptr(), 3 * w * h), "jpeg_amd_tensor_pixels_batch", ctx.handle)
    return out.view(n, h, w, 3)


def encode_tensors(ctx: Context, tensors, layout: Layout, quanta: Dict[int, Sequence[int]], source: _lib.TensorSource,
                   color=RGB) -> List[Spectral]:
    """Rectangular.encode for a batch of tensors in one call (jpeg_amd_encode_tensor_batch): tensors as in tensor_pixels,
    layout and quanta as in Rectangular.encode.  Returns one Spectral per image; their planes are views into one allocation
    per plane."""
    torch = _torch()
    n, w, h, stride = _source_args(ctx, tensors, source)
    tables, q = _encode_tables(layout, quanta)
    size = (w, h)
    units = layout.units(size)
    L = layout.c_layout(size, units, q)
    planes = [ctx.empty(n * 64 * ux * uy, torch.int16).view(n, uy, ux, 64) for ux, uy in units]
    dq = ctx.upload(np.stack(tables).astype(np.uint16))
    _lib.check(_lib.lib().jpeg_amd_encode_tensor_batch(
        ctx.handle, C.byref(L), n, tensors.data_ptr(), stride, C.byref(source), color.code, dq.data_ptr(), 0, len(tables),
        _ptrs(planes), _lib.size_array([64 * ux * uy for ux, uy in units])), "jpeg_amd_encode_tensor_batch", ctx.handle)
    return [Spectral(ctx, size, layout, [p[i] for p in planes], tables, q) for i in range(n)]


def compress_tensors(ctx: Context, tensors, layout: Layout, quanta: Dict[int, Sequence[int]], source: _lib.TensorSource, scans,
                     process: str = "baseline", metadata=None, threads: int = 0, color=RGB) -> List[bytes]:
    """Tensors to JPEG files in one call (jpeg_amd_compress_tensor_batch_device): the front launch and the fused encoder on the
    device, chunk by chunk, the entropy coding on `threads` host threads (0: all cores).  tensors as in tensor_pixels; layout,
    quanta, scans, process and metadata as in Rectangular.compress.  Returns the n files' bytes."""
    n, w, h, stride = _source_args(ctx, tensors, source)
    info = _lib.FrameInfo()
    info.width, info.height = w, h
    info.precision, info.ncomponents = layout.precision, layout.count
    info.process = {"baseline": 0, "extended": 1, "progressive": 2}[process]
    keys = []
    for p, (key, comp) in enumerate(zip(layout.recognized, layout.planes)):
        info.id[p] = int(key)
        info.factor_x[p], info.factor_y[p] = comp.factor
        keys.append(comp.qi)
    tkeys = sorted(set(keys))
    for k in tkeys:
        if k not in quanta:
            raise _lib.JpegAmdError(_lib.EINVAL, f"missing quantization table for quanta key {k}")
    tables = np.stack([np.asarray(quanta[k], np.uint16).reshape(64) for k in tkeys])
    qkey = (C.c_int32 * len(keys))(*keys)
    tk = (C.c_int32 * len(tkeys))(*tkeys)
    sarr = _scan_array(scans)
    marr, nmeta, _keep = _metadata_array(metadata)
    if n == 0:
        return []
    sizes = (C.c_size_t * n)()
    # sized generously (raw samples + headers), and the call repeated only if that was too small for some file
    cap = 3 * w * h * 2 + (1 << 16)
    for _ in range(2):
        out = np.empty((n, cap), np.uint8)
        st = _lib.lib().jpeg_amd_compress_tensor_batch_device(
            ctx.handle, C.byref(info), tensors.data_ptr(), stride, C.byref(source), n, color.code, qkey, tables.ctypes.data, tk,
            len(tkeys), sarr, len(scans), marr, nmeta, int(threads), out.ctypes.data, cap, sizes)
        if st == _lib.EINVAL and max(sizes) > cap:
            cap = max(sizes)
            continue
        _lib.check(st, "jpeg_amd_compress_tensor_batch_device", ctx.handle)
        break
    return [out[i, :sizes[i]].tobytes() for i in range(n)]


def _dedupe_q(layout: Layout) -> List[int]:
    """Spectral.set(quanta:) (decode.swift:2510-2543): one table per distinct quanta key,
    in plane order."""
    keys: List[int] = []
    q = []
    for c in layout.planes:
        if c.qi not in keys:
            keys.append(c.qi)
        q.append(keys.index(c.qi))
    return q


class Planar:
    """JPEG.Data.Planar<Format> (decode.swift:1480-1598): one uint16 plane
    [8*units_y, 8*units_x] per component (stored as int16 bit patterns)."""

    def __init__(self, ctx, size, layout, planes):
        self.ctx, self.size, self.layout, self.planes = ctx, (int(size[0]), int(size[1])), layout, list(planes)

    @classmethod
    def from_host(cls, ctx, size, layout, planes: Sequence[np.ndarray]):
        return cls(ctx, size, layout, [ctx.upload(np.asarray(p, np.uint16)) for p in planes])

    @property
    def units(self):
        return [(int(p.shape[1]) // 8, int(p.shape[0]) // 8) for p in self.planes]

    def interleaved(self, cosite: bool = False) -> "Rectangular":
        """Planar.interleaved(cosite:) -- decode.swift:4182-4276."""
        torch = _torch()
        L = self.layout.c_layout(self.size, self.units)
        W, H = self.size
        out = self.ctx.empty(W * H * self.layout.count, torch.int16)
        _lib.check(_lib.lib().jpeg_amd_planar_interleaved(
            self.ctx.handle, C.byref(L), _ptrs(self.planes), 1 if cosite else 0,
            out.data_ptr()), "jpeg_amd_planar_interleaved", self.ctx.handle)
        return Rectangular(self.ctx, self.size, self.layout, out.view(H, W, self.layout.count))

    def fdct(self, quanta: Dict[int, Sequence[int]]) -> Spectral:
        """Planar.fdct(quanta:) -- encode.swift:353-370.  quanta: {quanta key: 64 zigzag values}."""
        torch = _torch()
        keys: List[int] = []
        q = []
        for c in self.layout.planes:
            if c.qi not in quanta:
                # decode.swift:2527-2530 preconditionFailure("missing quantization table ...")
                raise _lib.JpegAmdError(_lib.EINVAL, f"missing quantization table for quanta key {c.qi}")
            if c.qi not in keys:
                keys.append(c.qi)
            q.append(keys.index(c.qi))
        tables = [np.asarray(quanta[k], np.uint16).reshape(64) for k in keys]
        L = self.layout.c_layout(self.size, self.units, q)
        out = [self.ctx.empty(64 * ux * uy, torch.int16).view(uy, ux, 64) for ux, uy in self.units]
        qarr, qptr = _quanta_array(tables)
        _lib.check(_lib.lib().jpeg_amd_planar_fdct(
            self.ctx.handle, C.byref(L), _ptrs(self.planes), qptr, len(tables), _ptrs(out)),
            "jpeg_amd_planar_fdct", self.ctx.handle)
        return Spectral(self.ctx, self.size, self.layout, out, tables, q)

    def host_planes(self) -> List[np.ndarray]:
        return [p.cpu().numpy().view(np.uint16) for p in self.planes]


class Rectangular:
    """JPEG.Data.Rectangular<Format> (decode.swift:1650-1718): interleaved uint16 samples
    [H, W, count] (stored as int16 bit patterns)."""

    def __init__(self, ctx, size, layout, values):
        self.ctx, self.size, self.layout, self.values = ctx, (int(size[0]), int(size[1])), layout, values
        # decode.swift:1710-1712
        if values.numel() != layout.count * self.size[0] * self.size[1]:
            raise _lib.JpegAmdError(_lib.EINVAL, "array count does not match size and layout")
        if self.size[0] <= 0 or self.size[1] <= 0:
            raise _lib.JpegAmdError(_lib.EINVAL, "size must be positive")

    @property
    def stride(self) -> int:
        return self.layout.count

    @classmethod
    def from_host(cls, ctx, size, layout, values: np.ndarray):
        return cls(ctx, size, layout, ctx.upload(np.asarray(values, np.uint16)))

    def unpack(self, color=RGB):
        """Rectangular.unpack(as:) -- decode.swift:4291-4298 -> uint8 tensor [H*W, 3]."""
        torch = _torch()
        n = self.size[0] * self.size[1]
        out = self.ctx.empty(3 * n, torch.uint8)
        _lib.check(_lib.lib().jpeg_amd_rectangular_unpack(
            self.ctx.handle, self.values.data_ptr(), n, self.layout.count, color.code,
            out.data_ptr()), "jpeg_amd_rectangular_unpack", self.ctx.handle)
        return out.view(-1, 3)

    @classmethod
    def decompress(cls, ctx: Context, source, cosite: bool = False) -> "Rectangular":
        """Rectangular.decompress(stream:cosite:) -- decode.swift:4367-4374:
        Spectral.decompress(...).idct().interleaved(cosite:)."""
        return Spectral.decompress(ctx, source).rectangular(cosite=cosite)

    @classmethod
    def pack(cls, ctx, size, layout, pixels, color=RGB) -> "Rectangular":
        """Rectangular.pack(size:layout:metadata:pixels:) -- encode.swift:453-464.
        pixels: uint8 [H*W, 3] (numpy or device tensor)."""
        torch = _torch()
        if isinstance(pixels, np.ndarray):
            pixels = ctx.upload(np.asarray(pixels, np.uint8))
        n = int(size[0]) * int(size[1])
        if pixels.numel() != 3 * n:
            raise _lib.JpegAmdError(_lib.EINVAL, "array count does not match size and layout")
        out = ctx.empty(n * layout.count, torch.int16)
        _lib.check(_lib.lib().jpeg_amd_rectangular_pack(
            ctx.handle, pixels.data_ptr(), n, layout.count, color.code, out.data_ptr()),
            "jpeg_amd_rectangular_pack", ctx.handle)
        return cls(ctx, size, layout, out.view(int(size[1]), int(size[0]), layout.count))

    def decomposed(self) -> Planar:
        """Rectangular.decomposed() -- encode.swift:389-425."""
        torch = _torch()
        units = self.layout.units(self.size)
        L = self.layout.c_layout(self.size, units)
        out = [self.ctx.empty(64 * ux * uy, torch.int16).view(8 * uy, 8 * ux) for ux, uy in units]
        _lib.check(_lib.lib().jpeg_amd_rectangular_decomposed(
            self.ctx.handle, C.byref(L), self.values.data_ptr(), _ptrs(out)),
            "jpeg_amd_rectangular_decomposed", self.ctx.handle)
        return Planar(self.ctx, self.size, self.layout, out)

    def spectral(self, quanta: Dict[int, Sequence[int]]) -> Spectral:
        """decomposed().fdct(quanta:) in one call (encode.swift:389-425, 353-370): one launch for formats whose planes lie at the
        image's scale or at half of it (jpeg_amd_rectangular_spectral), the staged kernels otherwise -- same coefficients."""
        torch = _torch()
        keys: List[int] = []
        q = []
        for c in self.layout.planes:
            if c.qi not in quanta:
                raise _lib.JpegAmdError(_lib.EINVAL, f"missing quantization table for quanta key {c.qi}")
            if c.qi not in keys:
                keys.append(c.qi)
            q.append(keys.index(c.qi))
        tables = [np.asarray(quanta[k], np.uint16).reshape(64) for k in keys]
        units = self.layout.units(self.size)
        L = self.layout.c_layout(self.size, units, q)
        out = [self.ctx.empty(64 * ux * uy, torch.int16).view(uy, ux, 64) for ux, uy in units]
        qarr, qptr = _quanta_array(tables)
        _lib.check(_lib.lib().jpeg_amd_rectangular_spectral(
            self.ctx.handle, C.byref(L), self.values.data_ptr(), qptr, len(tables), _ptrs(out)),
            "jpeg_amd_rectangular_spectral", self.ctx.handle)
        return Spectral(self.ctx, self.size, self.layout, out, tables, q)

    @classmethod
    def encode(cls, ctx, size, layout, pixels, quanta: Dict[int, Sequence[int]], color=RGB) -> Spectral:
        """Fused pack(...).decomposed().fdct(quanta:) -> Spectral."""
        torch = _torch()
        if isinstance(pixels, np.ndarray):
            pixels = ctx.upload(np.asarray(pixels, np.uint8))
        keys: List[int] = []
        q = []
        for c in layout.planes:
            if c.qi not in quanta:
                raise _lib.JpegAmdError(_lib.EINVAL, f"missing quantization table for quanta key {c.qi}")
            if c.qi not in keys:
                keys.append(c.qi)
            q.append(keys.index(c.qi))
        tables = [np.asarray(quanta[k], np.uint16).reshape(64) for k in keys]
        units = layout.units(size)
        L = layout.c_layout(size, units, q)
        out = [ctx.empty(64 * ux * uy, torch.int16).view(uy, ux, 64) for ux, uy in units]
        qarr, qptr = _quanta_array(tables)
        _lib.check(_lib.lib().jpeg_amd_encode(
            ctx.handle, C.byref(L), pixels.data_ptr(), color.code, qptr, len(tables), _ptrs(out)),
            "jpeg_amd_encode", ctx.handle)
        return Spectral(ctx, size, layout, out, tables, q)

    def compress(self, quanta: Dict[int, Sequence[int]], scans, process: str = "baseline", metadata=None,
                 path=None, restart_interval: int = 0) -> bytes:
        """Rectangular.compress(stream:quanta:) / compress(path:quanta:) -- encode.swift:2031,
        os.swift:412: decomposed().fdct(quanta:).compress(...)."""
        return self.spectral(quanta).compress(scans, process=process, metadata=metadata, path=path,
                                              restart_interval=restart_interval)

    def host_values(self) -> np.ndarray:
        return self.values.cpu().numpy().view(np.uint16)

    # ---- the one-call forms of the C ABI for custom formats (host memory in, host memory out) --------------------------------
    @staticmethod
    def decompress_to_host(ctx: Context, source, cosite: bool = False, recognized: int = 0, threads: int = 0):
        """Rectangular<Format>.decompress(stream:cosite:) for any JPEG.Format in ONE call of the C ABI
        (jpeg_amd_decompress_rectangular; decode.swift:4367-4374): -> (frame info, uint16 array [H, W, n]).
        recognized: how many of the frame's components the format recognises (0: all)."""
        data = np.frombuffer(_file_bytes(source), np.uint8)
        info = _lib.FrameInfo()
        _lib.check(_lib.lib().jpeg_amd_jpeg_inspect(data.ctypes.data, data.size, C.byref(info)), "jpeg_amd_jpeg_inspect")
        n = recognized or info.ncomponents
        out = np.empty((info.height, info.width, n), np.uint16)
        _lib.check(_lib.lib().jpeg_amd_decompress_rectangular(
            ctx.handle, data.ctypes.data, data.size, 1 if cosite else 0, recognized, threads, out.ctypes.data, out.size,
            C.byref(info)), "jpeg_amd_decompress_rectangular", ctx.handle)
        return info, out

    @staticmethod
    def compress_from_host(ctx: Context, size, layout: "Layout", values, quanta: Dict[int, Sequence[int]], scans,
                           process: str = "baseline", metadata=None, path=None, restart_interval: int = 0) -> bytes:
        """Rectangular<Format>.compress(stream:quanta:) for any JPEG.Format in ONE call of the C ABI
        (jpeg_amd_compress_rectangular; encode.swift:2031).  values: uint16 [H, W, count] in host memory."""
        values = np.ascontiguousarray(np.asarray(values, np.uint16).reshape(int(size[1]), int(size[0]), layout.count))
        info = _lib.FrameInfo()
        info.width, info.height = int(size[0]), int(size[1])
        info.precision, info.ncomponents = layout.precision, layout.count
        info.process = {"baseline": 0, "extended": 1, "progressive": 2}[process]
        info.restart_interval = int(restart_interval)
        keys = []
        for p, (key, comp) in enumerate(zip(layout.recognized, layout.planes)):
            info.id[p] = int(key)
            info.factor_x[p], info.factor_y[p] = comp.factor
            keys.append(comp.qi)
        tkeys = sorted(set(keys))
        for k in tkeys:
            if k not in quanta:
                raise _lib.JpegAmdError(_lib.EINVAL, f"missing quantization table for quanta key {k}")
        tables = np.stack([np.asarray(quanta[k], np.uint16).reshape(64) for k in tkeys])
        qkey = (C.c_int32 * len(keys))(*keys)
        tk = (C.c_int32 * len(tkeys))(*tkeys)
        sarr = _scan_array(scans)
        marr, nmeta, _keep = _metadata_array(metadata)
        n = C.c_size_t()
        # the entropy coder sizes its output from the coefficients: a first call without a buffer would run the kernels twice,
        # so the buffer is sized generously instead (raw samples + headers) and the call repeated only if that was too small
        cap = values.size * 2 + (1 << 16)
        for _ in range(2):
            out = np.empty(cap, np.uint8)
            st = _lib.lib().jpeg_amd_compress_rectangular(ctx.handle, C.byref(info), values.ctypes.data, qkey, tables.ctypes.data, tk,
                                                          len(tkeys), sarr, len(scans), marr, nmeta, out.ctypes.data, out.size, C.byref(n))
            if st == _lib.EINVAL and n.value > cap:
                cap = n.value
                continue
            _lib.check(st, "jpeg_amd_compress_rectangular", ctx.handle)
            break
        data = out[:n.value].tobytes()
        if path is not None:
            with open(path, "wb") as f:
                f.write(data)
        return data


def compression_quanta(kind: str, level: float) -> np.ndarray:
    """JPEG.CompressionLevel.quanta (encode.swift:260-333): host-side constant tables,
    64 values in zigzag order.  kind: 'luminance' | 'chrominance'."""
    lum = [16, 11, 10, 16, 124, 140, 151, 161, 12, 12, 14, 19, 126, 158, 160, 155,
           14, 13, 16, 24, 140, 157, 169, 156, 14, 17, 22, 29, 151, 187, 180, 162,
           18, 22, 37, 56, 168, 109, 103, 177, 24, 35, 55, 64, 181, 104, 113, 192,
           49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 199]
    chr_ = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
            24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
    key = lum if kind == "luminance" else chr_
    from .zigzag import ZIGZAG
    out = np.empty(64, np.uint16)
    for h in range(8):
        for k in range(8):
            v = 1.0 * (1 - level) + key[8 * h + k] * level
            v = float(np.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)  # .rounded(), Double
            out[ZIGZAG[h][k]] = int(max(1.0, min(v, 255.0)))
    return out
